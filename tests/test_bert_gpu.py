"""GPU suite of FrozenBERTEmbedder: attention with per-sample key lengths on exact-arithmetic inputs (tests/attn_varlen.py), gg_bert_embed
against torch fp32 on the CPU, the module against the reference's recorded outputs (tests/golden/bert.npz, make_golden_bert.py), the
conditioning's way through a DDIM chain, and a BERT-base-sized model against a CPU bf16 shadow.  Bounds: see each test; measured values
are printed and recorded in DESIGN.md 7l."""

import pytest
import torch
import torch.nn.functional as F

import attn_exact as X
import attn_varlen as V
import bert_ref
from test_bert_cpu import bert_ldm, make_dir, surf, tiny_cfg
from util import T, gold, rel_err, rms_err, seeded

pytestmark = pytest.mark.gpu
GG_ERR_BAD_SHAPE = -1
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return gold("bert")


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    return make_dir(tmp_path_factory.mktemp("bert_tiny_gpu"))


@pytest.fixture(scope="module")
def embedder(tiny, dev):
    from jointimagegeneration_amd import cond
    m = cond.FrozenBERTEmbedder(tiny, device=dev)
    m.bert_max_length = surf()["n_tok"]
    return m


def lens(case, dev, full=False):
    return torch.tensor([case.Tkv_max] * case.N if full else list(case.lengths), dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------ attention with key lengths
@pytest.mark.parametrize("regime", X.REGIMES)
@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_attention_kvlen_bit_exact(case, regime, dev):
    """One launch, samples of different lengths, poison past each length: the closed form of every length, bit for bit."""
    p = V.build(case, regime, dev)
    out = V.launch(case, p, lens(case, dev))
    bad = V.check_output(case, p, out)
    assert not bad, f"{case.name} [{regime}] lengths {case.lengths}: {bad}"


@pytest.mark.parametrize("case", V.F32_CASES, ids=lambda c: c.name)
def test_attention_kvlen_f32_bit_exact(case, dev):
    for regime in X.REGIMES:
        p = V.build(case, regime, dev, dtype=torch.float32, scale=X.F32_SCALE)
        out = V.launch(case, p, lens(case, dev))
        bad = V.check_output(case, p, out)
        assert not bad, f"{case.name} [{regime}] lengths {case.lengths}: {bad}"


@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_attention_kvlen_full_length_equals_the_plain_entry(case, dev):
    """kv_len = Tkv for every sample: bit-equal to gg_attention_forward on the same buffers (poison rows and all: they are live here)."""
    assert X.plan_of(case.full())[1:3] == (1, 0)                                   # the plain entry runs the plain kernel on these shapes
    for regime in ("sel", "grp"):
        p = V.build(case, regime, dev)
        a, b = V.launch(case, p, lens(case, dev, full=True)), V.launch(case, p, None)
        assert bool(torch.isfinite(X.out_view(case.full(), b).float()).all())
        assert not X.mismatches(a, b), X.mismatches(a, b)
        assert X.mismatches(X.out_view(case.full(), b), p.want.to(dev))              # ... and the poison does show when it is live


# ------------------------------------------------------------------------------------------------ gg_bert_embed
def raw_bert_embed(ids, tts, tabs, eps, stride, dev, host=True):
    """gg_bert_embed at the C-ABI into a sentinel-filled buffer with 64 elements of slack; returns (rc, rows [R, stride], slack)."""
    from jointimagegeneration_amd import _lib
    word, pos, typ, gamma, beta = (t.to(dev) for t in tabs)
    R, T_len = ids.numel(), ids.shape[1]
    buf = torch.full((R * stride + 64,), SENTINEL, dtype=torch.bfloat16, device=dev)
    ids32, tts32 = ids.int().contiguous(), (tts.int().contiguous() if tts is not None else None)
    ids_d, tts_d = ids32.to(dev), (tts32.to(dev) if tts is not None else None)
    rc = _lib.load().gg_bert_embed(ids_d.data_ptr(), tts_d.data_ptr() if tts is not None else None, R, T_len, word.data_ptr(), word.shape[0],
                                   pos.data_ptr(), pos.shape[0], typ.data_ptr(), typ.shape[0], word.shape[1], gamma.data_ptr(), beta.data_ptr(),
                                   eps, buf.data_ptr(), stride, ids32.data_ptr() if host else None,
                                   tts32.data_ptr() if host and tts is not None else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, buf[:R * stride].view(R, stride).cpu(), buf[R * stride:].cpu()


@pytest.mark.parametrize("shape, D", [((3, 16), 64), ((2, 5), 48)])
def test_bert_embed_against_torch_fp32(dev, shape, D):
    """LayerNorm(word[ids] + type[tt] + pos[t]) against torch fp32 on the CPU.  Bound of the gg_layernorm_rows test (test_cond_gpu.py): the
    one rounding to bf16 (2^-8 |y|) plus fp32 arithmetic on terms of size max|gamma| max|xhat| + max|beta| (1e-5 of it).  Pad lanes zero
    (16 at D = 48, none at 64), the memory after the last row untouched."""
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(D)
    V_, P, NT, eps = 97, 20, 2, 1e-12
    word, pos, typ = torch.randn(V_, D, generator=gen), torch.randn(P, D, generator=gen), torch.randn(NT, D, generator=gen)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=gen), 0.05 * torch.randn(D, generator=gen)
    ids = torch.randint(0, V_, shape, generator=gen)
    ids.view(-1)[0], ids.view(-1)[1] = V_ - 1, 0
    stride = ops.pad32(D)
    for tts in (None, torch.randint(0, NT, shape, generator=gen)):
        x = word[ids] + typ[tts if tts is not None else torch.zeros_like(ids)] + pos[:shape[1]]
        ref = F.layer_norm(x, (D,), gamma, beta, eps)
        xhat = F.layer_norm(x, (D,), None, None, eps)
        rc, rows, slack = raw_bert_embed(ids, tts, (word, pos, typ, gamma, beta), eps, stride, dev)
        assert rc == 0
        err = (rows[:, :D].float().view(*shape, D) - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * float(gamma.abs().max() * xhat.abs().max() + beta.abs().max())
        print(f"gg_bert_embed {shape} x {D}: max err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), float((err - bound).max())
        assert bool((rows[:, D:] == 0).all()) and bool((slack == SENTINEL).all())
    got = ops.bert_embed(ids.int().to(dev), None, word.to(dev), pos.to(dev), typ.to(dev), gamma.to(dev), beta.to(dev), eps, ids_host=ids.int())
    assert tuple(got.shape) == (shape[0], 1, 1, shape[1], stride)
    assert torch.equal(got.cpu().view(-1, stride), raw_bert_embed(ids, None, (word, pos, typ, gamma, beta), eps, stride, dev)[1])


def test_bert_embed_ids_outside_the_table(dev):
    from jointimagegeneration_amd import _lib, ops
    gen = torch.Generator().manual_seed(5)
    D = 48
    tabs = (torch.randn(97, D, generator=gen), torch.randn(20, D, generator=gen), torch.randn(2, D, generator=gen), torch.ones(D), torch.zeros(D))
    ids = torch.tensor([[5, 97, 96]])
    rc, rows, slack = raw_bert_embed(ids, None, tabs, 1e-12, 64, dev)
    assert rc == GG_ERR_BAD_SHAPE and b"token id 97" in _lib.load().gg_last_error()
    assert bool((rows == SENTINEL).all()) and bool((slack == SENTINEL).all())          # refused before the launch
    assert raw_bert_embed(torch.tensor([[5, -1, 96]]), None, tabs, 1e-12, 64, dev)[0] == GG_ERR_BAD_SHAPE
    assert raw_bert_embed(torch.tensor([[5, 6, 96]]), torch.tensor([[0, 2, 0]]), tabs, 1e-12, 64, dev)[0] == GG_ERR_BAD_SHAPE        # token type
    assert raw_bert_embed(torch.zeros(1, 21, dtype=torch.long), None, tabs, 1e-12, 64, dev)[0] == GG_ERR_BAD_SHAPE                  # T > P
    assert raw_bert_embed(ids.clamp(max=96), None, tabs, 1e-12, 32, dev)[0] == GG_ERR_BAD_SHAPE                                    # stride < D
    # without the host copies nothing can be checked: a zero row, nothing read, as gg_embed_rows
    rc, rows, slack = raw_bert_embed(ids, None, tabs, 1e-12, 64, dev, host=False)
    ok, _, _ = raw_bert_embed(ids.clamp(max=96), None, tabs, 1e-12, 64, dev)[1], None, None
    assert rc == 0 and bool((rows[1] == 0).all()) and torch.equal(rows[0], ok[0]) and torch.equal(rows[2], ok[2]) and bool((slack == SENTINEL).all())
    with pytest.raises(RuntimeError, match="token id 97"):
        ops.bert_embed(ids.int().to(dev), None, *(t.to(dev) for t in tabs), 1e-12, ids_host=ids.int())


# ------------------------------------------------------------------------------------------------ the module against the reference
@pytest.mark.parametrize("copy", ["ccdm", "ldm"])
def test_embedder_matches_both_reference_copies(dev, g, embedder, copy):
    """bf16 network with fp32 accumulation: rel_err < 3e-2, the token-embedder bound of tests/test_cond_gpu.py.  x = 1 on a batch of 3,
    x = 2 under use_text_split (every text becomes [text, ""], chunk xi on rows xi::x)."""
    s, m = surf(), embedder
    m.use_text_split, m.bert_encode_batch = False, 1
    z1 = m.encode([s["strings"][i] for i in s["batch3"]])
    e1 = rel_err(z1, T(g[f"{copy}_x1"]))
    m.use_text_split, m.bert_encode_batch = True, 2
    try:
        z2 = m.encode([s["strings"][i] for i in s["split"]])
    finally:
        m.use_text_split, m.bert_encode_batch = False, 1
    e2 = rel_err(z2, T(g[f"{copy}_x2"]))
    print(f"FrozenBERTEmbedder vs the {copy} copy: x = 1 rel_err {e1:.3e}, x = 2 rel_err {e2:.3e}")
    assert z1.dtype == torch.float32 and tuple(z1.shape) == (3, 16, 64) and tuple(z2.shape) == (2, 32, 64)
    assert e1 < 3e-2 and e2 < 3e-2


def test_padding_is_invisible_and_padded_rows_are_finite(dev, g, embedder):
    """Outputs at valid positions are bit-equal when the ids under the padding change; padded rows are finite; encode(list of str)
    equals encode(tokens, attention_mask)."""
    s, m = surf(), embedder
    ids, mask = T(g["ids"]).long(), T(g["mask"]).long()
    z_text = m.encode(s["strings"])
    z_tok = m.encode(ids.to(dev), attention_mask=mask.to(dev))
    assert torch.equal(z_text, z_tok) and bool(torch.isfinite(z_text).all())
    other = torch.where(mask.bool(), ids, (ids * 7 + torch.arange(ids.shape[1])[None] * 13 + 5) % 97)
    assert bool((other != ids)[~mask.bool()].any())
    z_other = m.encode(other.to(dev), attention_mask=mask.to(dev))
    valid = mask.bool().to(dev)
    assert torch.equal(z_other[valid], z_tok[valid]) and bool(torch.isfinite(z_other).all())
    assert not torch.equal(z_other[~valid], z_tok[~valid])                           # the padded rows themselves do depend on their ids
    with pytest.raises(NotImplementedError, match="not a prefix"):
        m.encode(ids.to(dev), attention_mask=mask.flip(1).to(dev))
    with pytest.raises(RuntimeError, match="token id 128"):
        m.encode(torch.full((1, 16), 128, device=dev), attention_mask=torch.ones(1, 16, dtype=torch.long, device=dev))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.encode(torch.zeros(1, 41, dtype=torch.long, device=dev), attention_mask=torch.ones(1, 41, dtype=torch.long, device=dev))
    with pytest.raises(RuntimeError, match="cpu"):
        m.encode(ids, attention_mask=mask)


def test_cli_writes_the_features_preloaded_bert_encoder_takes(dev, tmp_path):
    """python -m jointimagegeneration_amd.cond (its main(), in this process) at the real length of 512 tokens: [b, hidden, length] fp32,
    equal to encode() transposed, and within the module bound of bert_ref on the rows below each length."""
    import numpy as np
    from jointimagegeneration_amd import cond
    s = surf()
    cfg = tiny_cfg(max_position_embeddings=512)
    d = make_dir(tmp_path / "bert512", cfg=cfg)
    tf = tmp_path / "texts.txt"
    tf.write_text(s["strings"][3] + "\n" + s["strings"][4] + "\n", encoding="utf-8")
    out = str(tmp_path / "feats.npy")
    assert cond._main(["--bert", d, "--text", s["strings"][1], "--text-file", str(tf), "--out", out]) == 0
    feats = torch.from_numpy(np.load(out))
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (3, 64, 512)
    m = cond.FrozenBERTEmbedder(d, device=dev)
    texts = [s["strings"][i] for i in (1, 3, 4)]
    assert torch.equal(m.encode(texts).permute(0, 2, 1).cpu(), feats)
    ids, mask = m.tokenizer.encode(texts, 512)
    lengths = torch.tensor(mask).sum(1)
    ref = bert_ref.forward(bert_ref.seeded_state_dict(cfg, "bert_tiny."), torch.tensor(ids), lengths, cfg)
    valid = torch.arange(512)[None, :] < lengths[:, None]
    e = rel_err(feats.permute(0, 2, 1)[valid], ref[valid])
    print(f"cond CLI at 512 tokens: rel_err {e:.3e} on the rows below each length")
    assert e < 3e-2 and bool(torch.isfinite(feats).all())


# ------------------------------------------------------------------------------------------------ chain
def test_ddim_chain_with_frozen_bert_vs_reference(dev, g, tiny):
    """3 DDIM steps, eta = 0, conditioning = get_learned_conditioning(list of str), against the reference's chain.  Metric and bound of the
    cond chain of tests/test_cond_gpu.py (max 2e-2, rms 1.5e-2 of the reference).  The captured chain equals the eager one bit for bit."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    s = surf()
    m = seeded(bert_ldm(tiny), "ldm_bert.").to(dev)
    x_T = T(g["chain_x_T"]).to(dev)
    c = m.get_learned_conditioning([s["strings"][i] for i in s["chain"]])
    ec = rel_err(c, T(g["chain_c"]))
    assert tuple(c.shape) == (2, 16, 64) and ec < 3e-2
    smp = DDIMSampler(m)
    run = lambda sm, cc: sm.sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=cc, verbose=False, x_T=x_T, dims=2, eta=0.0)[0]
    z = run(smp, c)
    assert list(smp.ddim_timesteps) == list(g["chain_ddim_timesteps"])
    e, r = rel_err(z, T(g["chain_z"])), rms_err(z, T(g["chain_z"]))
    print(f"bert chain: conditioning rel_err {ec:.3e}; z max {e:.3e} rms {r:.3e} (of the reference's)")
    assert e < 2e-2 and r < 1.5e-2
    z2 = run(smp, c)                                                                # the captured graph, replayed on reloaded inputs
    assert any(st["graph"] is not None for st in smp._graphs.values()) and torch.equal(z, z2)
    eager = DDIMSampler(m)
    eager.use_graph = False
    assert torch.equal(run(eager, c), z)


# ------------------------------------------------------------------------------------------------ BERT-base width
def test_bert_base_width_within_twice_the_bf16_shadow(dev):
    """12 layers x 768 (12 heads of 64) x 3072, vocab 21128, T = 128, N = 2 with lengths 128 and 37, seed-recipe weights.  Reference:
    bert_ref in fp32 on the CPU, rows below each sample's length.  The bound is not a fixed number: a CPU shadow of bert_ref with the
    engine's storage roundings (Linear weights and every stored activation through bf16) has its own rel_err against the same reference,
    and the engine must stay within TWICE that (a different fp32 accumulation order, the exp2 softmax, P rounded to bf16 before P V).
    Measured: see DESIGN.md 7l."""
    from jointimagegeneration_amd import cond
    cfg, lengths = bert_ref.BASE, [128, 37]
    sd = bert_ref.seeded_state_dict(cfg, "bert_base.")
    gen = torch.Generator().manual_seed(12)
    ids = torch.randint(0, cfg["vocab_size"], (2, 128), generator=gen)
    ids[0, 0], ids[1, 1] = cfg["vocab_size"] - 1, 0
    ref = bert_ref.forward(sd, ids, lengths, cfg)
    shadow = bert_ref.shadow_bf16(sd, ids, lengths, cfg)
    m = cond.BertModel(cfg)
    m.load_state_dict(sd)
    m = m.eval().to(dev)
    with torch.no_grad():
        got = m.run(ids.int().to(dev), lengths, ids_host=ids.int().contiguous()).cpu()
    valid = torch.arange(128)[None, :] < torch.tensor(lengths)[:, None]
    e_eng, e_sh = rel_err(got[valid], ref[valid]), rel_err(shadow[valid], ref[valid])
    r_eng, r_sh = rms_err(got[valid], ref[valid]), rms_err(shadow[valid], ref[valid])
    print(f"BERT-base width: engine rel_err {e_eng:.3e} (rms {r_eng:.3e}), bf16 shadow rel_err {e_sh:.3e} (rms {r_sh:.3e}), "
          f"ratio {e_eng / e_sh:.2f}; max |ref| {float(ref[valid].abs().max()):.2f}")
    assert bool(torch.isfinite(got).all())
    assert e_eng <= 2.0 * e_sh, (e_eng, e_sh)
