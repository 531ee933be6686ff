"""CPU suite: the shadow harness (tests/shadow.py) itself.  Its fp64 references equal torch's CPU operators (F.conv2d / conv3d,
F.group_norm, scaled-dot-product attention, in fp64) to 1e-12 on small shapes with every conv feature production uses, and its
comparator passes a clean kernel-like output (the reference rounded to the kernel's output type) but fails on each injected defect.
The same for the families of the text, 3-D, GAN and LPIPS networks (F.gelu, F.layer_norm, F.embedding, F.interpolate, F.conv2d /
conv3d(k=4, padding=2) + leaky_relu, F.max_pool2d(F.relu(.)), attention under a key mask, torch.cdist(...).argmin), one planted
violation per rule of the operand contract, and the completeness check: every `ops.X(` call of the network modules is wrapped by the
shadow or listed, with a reason, in its EXEMPT table."""
import math

import pytest
import torch
import torch.nn.functional as F

import shadow as SH

torch.set_grad_enabled(False)
REF_TOL = 1e-12


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cl(N, sp, C, seed, cpad=None):
    """random bf16 channels-last tensor [N, D, H, W, Cpad] with zero pad lanes"""
    cp = cpad or SH.pad32(C)
    t = torch.zeros((N,) + tuple(sp) + (cp,), dtype=torch.bfloat16)
    t[..., :C] = torch.randn((N,) + tuple(sp) + (C,), generator=gen(seed)).to(torch.bfloat16)
    return t


def ncdhw(t):
    return t.double().permute(0, 4, 1, 2, 3)


def torch_conv(call: SH.ConvCall, pad_prologue_bug=False, up_shift=False, bias_swap=False):
    """The same conv through F.conv3d in fp64 (channels-last [N, Do, Ho, Wo, Cout_w] result, before any GEGLU / rounding).
    The flags inject the defects of the mutation tests."""
    x = ncdhw(torch.cat(call.srcs, -1))
    N = x.shape[0]
    cin = x.shape[1]
    k = call.k
    if call.upsample:
        for dim, kk in zip((2, 3, 4), k):
            if kk == 3:
                x = x.repeat_interleave(2, dim)
                if up_shift:                                        # off-by-one source index: (i + 1) // 2
                    x = torch.cat([x.narrow(dim, 1, x.shape[dim] - 1), x.narrow(dim, x.shape[dim] - 1, 1)], dim)
    pads = []
    for kk in reversed(k):
        pads += [0, 0] if kk == 1 else ([call.pad, call.pad] if call.pad == 1 else [0, 1])
    if call.prologue is not None:
        s = call.prologue[0].double()[:, :, None, None, None]
        t = call.prologue[1].double()[:, :, None, None, None]
        if pad_prologue_bug:
            x = F.pad(x, pads)                                      # activation applied to the zero padding too
            x = x * s + t
            x = SH.silu(x) if call.act else x
        else:
            x = x * s + t
            x = SH.silu(x) if call.act else x
            x = F.pad(x, pads)
    else:
        x = F.pad(x, pads)
    W = call.w.to(torch.bfloat16).double()
    Cw = W.shape[0]
    Wf = torch.zeros((Cw, cin, W.shape[2]), dtype=torch.float64)
    Wf[:, :W.shape[1]] = W
    y = F.conv3d(x, Wf.reshape(Cw, cin, *k), stride=call.stride)
    if call.skip is not None:
        xs = ncdhw(torch.cat(call.skip[0], -1))
        Ws = torch.zeros((Cw, xs.shape[1], 1, 1, 1), dtype=torch.float64)
        Ws[:, :call.skip[1].shape[1], 0, 0, 0] = call.skip[1].to(torch.bfloat16).double()[:, :, 0]
        y = y + F.conv3d(xs, Ws)
    y = y.permute(0, 2, 3, 4, 1)
    cp = SH.pad32(Cw)
    if call.bias is not None:
        b = call.bias.double().reshape(-1, cp)[:, :Cw]
        rows = b[torch.arange(N)] if call.bias_per_sample else b[:1].expand(N, -1)
        if bias_swap:
            rows = rows[[1, 0] + list(range(2, N))]
        y = y + rows[:, None, None, None, :]
    if call.residual is not None:
        y = y + call.residual[..., :Cw].double()
    return y


def kernel_like(call, y, dtype=torch.bfloat16):
    """A kernel-style output tensor: y (fp64 [N, Do, Ho, Wo, Cout_w]) with the GEGLU applied, rounded, in a zero-padded CL buffer."""
    if call.geglu:
        inner = y.shape[-1] // 2
        j = torch.arange(inner)
        y = y[..., (j // 16) * 32 + j % 16] * SH.gelu(y[..., (j // 16) * 32 + 16 + j % 16])
        cp = inner
    else:
        cp = SH.pad32(y.shape[-1])
    out = torch.zeros(tuple(y.shape[:-1]) + (cp,), dtype=dtype)
    out[..., :y.shape[-1]] = y.to(dtype)
    return out


def make_call(feature, N=2, seed=0):
    """Small conv calls covering every conv feature of the production networks."""
    g = gen(seed + 100)
    rnd = lambda *s: torch.randn(*s, generator=g)
    two_d = feature not in ("prologue3d", "affine3d", "prologue_acc3d", "up3d", "plain3d")
    sp = (1, 9, 10) if two_d else (4, 5, 6)
    k = (1, 3, 3) if two_d else (3, 3, 3)
    c1, cout = 32, 40
    srcs = [cl(N, sp, c1, seed)]
    kw = dict(k=k)
    if feature == "two_sources":
        srcs.append(cl(N, sp, 24, seed + 1))
    if feature in ("one_by_one", "geglu"):
        kw["k"], kw["pad"] = (1, 1, 1), 0
    if feature == "geglu":
        cout = 64
        kw["geglu"] = True
    if feature in ("upsample", "up3d"):
        kw["upsample"] = True
    if feature == "stride2":
        kw["stride"] = 2
    if feature == "stride2_pad0":
        kw["stride"], kw["pad"] = 2, 0
    cin = sum(s.shape[-1] for s in srcs)
    ntaps = kw["k"][0] * kw["k"][1] * kw["k"][2]
    cin_log = c1 + (24 if feature == "two_sources" else 0)
    w = rnd(cout, cin_log, ntaps) * 0.1
    per_sample = feature in ("bias_per_sample", "residual", "two_sources")
    bias = torch.zeros((N if per_sample else 1) * SH.pad32(cout))
    bias.view(-1, SH.pad32(cout))[:, :cout] = rnd(N if per_sample else 1, cout)
    call = SH.ConvCall(srcs=srcs, w=w, bias=bias, bias_per_sample=per_sample, cout=cout, **kw)
    out_sp = call.out_extent
    if feature == "residual":
        call.residual = cl(N, out_sp, cout, seed + 2)
    if feature in ("prologue2d", "prologue3d", "affine3d", "up3d"):
        call.prologue = (1.0 + 0.3 * rnd(N, cin), 0.5 + 0.5 * rnd(N, cin))
        call.act = feature != "affine3d"
    if feature == "prologue_acc3d":
        gamma, beta = 1.0 + 0.2 * rnd(cin), 0.3 + 0.2 * rnd(cin)
        sc, sh, dsc, dsh = SH.gn_reference(srcs, c1, gamma, beta, 1e-5)
        call.prologue, call.prologue_err = (sc, sh), (dsc, dsh)
        call.gn = (gamma, beta)
    if feature == "skip":
        call.skip = ([cl(N, sp, 32, seed + 3), cl(N, sp, 16, seed + 4)], rnd(cout, 48, 1) * 0.1)
    if feature == "ddim":
        call.w, call.cout = rnd(4, cin_log, ntaps) * 0.1, 4
        call.bias = torch.zeros(32)
        call.ddim = (rnd(N * out_sp[0] * out_sp[1] * out_sp[2], 4), torch.tensor([0.3, 0.5, 0.0, math.sqrt(0.7)]))
    return call


FEATURES = ["plain2d", "plain3d", "two_sources", "residual", "bias_per_sample", "upsample", "up3d", "stride2", "stride2_pad0",
            "prologue2d", "prologue3d", "affine3d", "prologue_acc3d", "skip", "one_by_one", "geglu", "ddim"]


@pytest.mark.parametrize("feature", FEATURES)
def test_conv_reference_equals_torch_conv(feature):
    call = make_call(feature)
    y = torch_conv(call)
    N = y.shape[0]
    sp = tuple(y.shape[1:4])
    for n in range(N):
        pos = SH._all_positions(sp)
        ref, bound = SH.conv_reference(call, n, pos)
        want = y[n][pos[:, 0], pos[:, 1], pos[:, 2]]
        if call.geglu:
            want = kernel_like(call, y[n:n + 1], torch.float64)[0][pos[:, 0], pos[:, 1], pos[:, 2]]
        assert float((ref - want).abs().max()) <= REF_TOL * float(want.abs().max())
        assert bool((bound > 0).all())
    # a clean kernel-like output passes the comparator, fp32 and bf16
    dtype = torch.float32 if feature == "ddim" else torch.bfloat16
    got = kernel_like(call, y, dtype)
    ddim_got = None
    if call.ddim is not None:
        x0, sc = call.ddim
        a_t, a_p, sig, s1m = (float(v) for v in sc.double())
        e = y.reshape(-1, y.shape[-1]).double()[:, :4]
        px0 = (x0.double() - s1m * e) / math.sqrt(a_t)
        xn = math.sqrt(a_p) * px0 + math.sqrt(1 - a_p - sig * sig) * e
        ddim_got = (xn.float(), px0.float(), xn.to(torch.bfloat16))
    r, r_dd, samples = SH.conv_ratio(call, got, 0, ddim_got)
    assert samples == N and r <= 1.0, r
    if call.ddim is not None:
        assert r_dd <= 1.0, r_dd
        bad = (ddim_got[0].clone(), ddim_got[1], ddim_got[2])
        bad[0][-1, 3] += 1.0
        assert SH.conv_ratio(call, got, 0, bad)[1] > 1.0


def test_groupnorm_reference_equals_group_norm():
    N, sp = 3, (2, 5, 7)
    a, b = cl(N, sp, 64, 1), cl(N, sp, 40, 2, cpad=64)
    gamma, beta = 1.0 + 0.2 * torch.randn(104, generator=gen(3)), 0.2 * torch.randn(104, generator=gen(4))
    sc, sh, dsc, dsh = SH.gn_reference([a, b], 96, gamma, beta, 1e-5)
    x = ncdhw(torch.cat([a, b], -1))[:, :96]
    want = F.group_norm(x, 32, gamma[:96].double(), beta[:96].double(), 1e-5)
    got = x * sc[:, :96, None, None, None] + sh[:, :96, None, None, None]
    assert float((got - want).abs().max()) <= REF_TOL * float(want.abs().max())
    assert float(sc[:, 96:].abs().max()) == 0.0 and bool((dsc[:, :96] > 0).all())


def test_attention_reference_equals_sdpa_and_views_match_layouts():
    N, T, heads, hd = 2, 50, 3, 32
    C = heads * hd
    qkv = torch.randn(N, 1, 1, T, 3 * C, generator=gen(5)).to(torch.bfloat16)
    # legacy order: per head [q | k | v] blocks of hd
    qv = SH.attention_view(qkv, N, T, heads, hd, 3 * C, 3 * hd, 0)
    kv = SH.attention_view(qkv, N, T, heads, hd, 3 * C, 3 * hd, hd)
    vv = SH.attention_view(qkv, N, T, heads, hd, 3 * C, 3 * hd, 2 * hd)
    r = qkv.reshape(N, T, heads, 3, hd)
    assert torch.equal(qv, r[:, :, :, 0]) and torch.equal(kv, r[:, :, :, 1]) and torch.equal(vv, r[:, :, :, 2])
    scale = hd ** -0.5
    want = F.scaled_dot_product_attention(qv.double().transpose(1, 2), kv.double().transpose(1, 2), vv.double().transpose(1, 2),
                                          scale=scale).transpose(1, 2)
    for n in range(N):
        for h in range(heads):
            ref, _ = SH.attention_reference(qv[n, :, h], kv[n, :, h], vv[n, :, h], scale)
            assert float((ref - want[n, :, h]).abs().max()) <= REF_TOL * float(want.abs().max())
    out = torch.zeros(N, 1, 1, T, C, dtype=torch.bfloat16)
    ov = SH.attention_view(out, N, T, heads, hd, C, hd, 0)
    ov.copy_(want.to(torch.bfloat16))
    assert SH.attention_ratio(qv, kv, vv, ov, scale) <= 1.0
    ov[1, T - 1, heads - 1, hd - 1] += 0.05
    assert SH.attention_ratio(qv, kv, vv, ov, scale) > 1.0


def test_positions_cover_every_edge_corner_and_face():
    p = SH.sample_positions((1, 72, 72), 0)
    per = {(0, h, w) for h in range(72) for w in range(72) if h in (0, 71) or w in (0, 71)}
    got = {tuple(v) for v in p.tolist()}
    assert per <= got and len(got) >= len(per) + 1500
    p3 = {tuple(v) for v in SH.sample_positions((20, 20, 20), 1).tolist()}
    edges = {(d, h, w) for d in range(20) for h in range(20) for w in range(20)
             if sum(c in (0, 19) for c in (d, h, w)) >= 2}
    assert edges <= p3
    for i in range(3):
        for v in (0, 19):
            assert sum(1 for q in p3 if q[i] == v) > 200


# ------------------------------------------------------------------------------------------------ mutation checks
def _ratio_of(call, got):
    return SH.conv_ratio(call, got, 0)[0]


@pytest.mark.parametrize("feature", ["plain2d", "prologue3d", "upsample", "bias_per_sample"])
def test_wrong_last_corner_of_last_sample_fails(feature):
    call = make_call(feature, N=3)
    got = kernel_like(call, torch_conv(call))
    assert _ratio_of(call, got) <= 1.0
    got[-1, -1, -1, -1, call.cout - 1] += 0.1 * float(got.float().abs().max())      # 10 % of the output's scale, one element
    assert _ratio_of(call, got) > 1.0


def test_wrong_corner_fails_where_positions_are_sampled():
    call = make_call("plain2d", N=2)
    call.srcs = [cl(2, (1, 72, 72), 32, 9)]
    got = kernel_like(call, torch_conv(call))
    assert _ratio_of(call, got) <= 1.0
    got[-1, 0, 71, 71, 0] += 0.25
    assert _ratio_of(call, got) > 1.0


def test_nonzero_pad_lane_fails():
    call = make_call("plain2d")
    got = kernel_like(call, torch_conv(call))
    assert got.shape[-1] > call.cout and _ratio_of(call, got) <= 1.0
    got[0, 0, 3, 3, call.cout + 5] = 2.0 ** -20
    assert _ratio_of(call, got) == math.inf


@pytest.mark.parametrize("feature", ["prologue2d", "prologue3d", "up3d"])
def test_prologue_applied_to_zero_padding_fails(feature):
    call = make_call(feature)
    assert _ratio_of(call, kernel_like(call, torch_conv(call))) <= 1.0
    assert _ratio_of(call, kernel_like(call, torch_conv(call, pad_prologue_bug=True))) > 1.0


def test_swapped_per_sample_bias_rows_fail():
    call = make_call("bias_per_sample")
    assert _ratio_of(call, kernel_like(call, torch_conv(call))) <= 1.0
    assert _ratio_of(call, kernel_like(call, torch_conv(call, bias_swap=True))) > 1.0


def test_swapped_film_rows_fail():
    N, C = 3, 64
    g = gen(11)
    scale, shift = torch.randn(N, 96, generator=g), torch.randn(N, 96, generator=g)
    film = torch.randn(N, 2 * C + 8, generator=g)

    def fold(f):
        s, t = scale.clone(), shift.clone()
        s[:, :C] = (scale[:, :C].double() * (1 + f[:, :C].double())).float()
        t[:, :C] = (shift[:, :C].double() * (1 + f[:, :C].double()) + f[:, C:2 * C].double()).float()
        return s, t
    assert SH.film_ratio(scale, shift, film, C, *fold(film)) <= 1.0
    assert SH.film_ratio(scale, shift, film, C, *fold(film[[1, 0, 2]])) > 1.0
    s, t = fold(film)
    t[0, C] += 1.0                                                 # a channel beyond C must stay as it was
    assert SH.film_ratio(scale, shift, film, C, s, t) == math.inf


def test_off_by_one_upsample_index_fails():
    for feature in ("upsample", "up3d"):
        call = make_call(feature)
        assert _ratio_of(call, kernel_like(call, torch_conv(call))) <= 1.0
        assert _ratio_of(call, kernel_like(call, torch_conv(call, up_shift=True))) > 1.0


def test_groupnorm_statistics_from_the_wrong_sample_fail():
    N, sp, Cc = 3, (2, 6, 6), 128
    x = cl(N, sp, Cc, 21)
    x[1] = (x[1].float() * 1.5 + 0.4).to(torch.bfloat16)                # samples with different statistics
    gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=gen(22)), 0.2 * torch.randn(Cc, generator=gen(23))
    sc, sh, dsc, dsh = SH.gn_reference([x], Cc, gamma, beta, 1e-5)
    clean_s, clean_t = sc.float(), sh.float()
    assert SH.coeff_ratio(clean_s, clean_t, sc, sh, dsc, dsh, Cc) <= 1.0
    # group 3 (channels 12..15) of sample 1 normalised with sample 0's mean / rstd
    xs = ncdhw(x)
    g = slice(12, 16)
    mean0 = xs[0, g].mean()
    rstd0 = 1.0 / torch.sqrt(xs[0, g].var(unbiased=False) + 1e-5)
    bad_s, bad_t = clean_s.clone(), clean_t.clone()
    bad_s[1, g] = (rstd0 * gamma[g].double()).float()
    bad_t[1, g] = (beta[g].double() - mean0 * rstd0 * gamma[g].double()).float()
    assert SH.coeff_ratio(bad_s, bad_t, sc, sh, dsc, dsh, Cc) > 1.0
    # the same defect inside a fused normalise kernel's output
    for act in (True, False):
        z = xs * clean_s.double()[:, :, None, None, None] + clean_t.double()[:, :, None, None, None]
        zb = xs * bad_s.double()[:, :, None, None, None] + bad_t.double()[:, :, None, None, None]
        f = SH.silu if act else (lambda v: v)
        good = f(z).permute(0, 2, 3, 4, 1).to(torch.bfloat16)
        bad = f(zb).permute(0, 2, 3, 4, 1).to(torch.bfloat16)
        assert SH.apply_ratio([x], sc, sh, dsc, dsh, act, good, Cc) <= 1.0
        assert SH.apply_ratio([x], sc, sh, dsc, dsh, act, bad, Cc) > 1.0


def test_conv_epilogue_statistics_check():
    N, sp, cout = 2, (1, 8, 8), 40
    y = cl(N, sp, cout, 31)
    m = SH.channel_moments(y)
    acc = torch.zeros((N, 32, 64, 2), dtype=torch.int64)
    q = torch.stack([torch.round(m[0] * SH.ACC_SUM_SCALE), torch.round(m[1] * SH.ACC_SQ_SCALE)], -1).long()
    acc[:, 5] = q                                                 # any stripe: the consumer sums them
    assert SH.acc_ratio(y, cout, acc) <= 1.0
    bad = acc.clone()
    bad[1, 5, 7], bad[0, 5, 7] = acc[0, 5, 7], acc[1, 5, 7]           # one channel's sums from the other sample
    assert SH.acc_ratio(y, cout, bad) > 1.0
    bad = acc.clone()
    bad[0, 0, cout + 1, 0] = 1
    assert SH.acc_ratio(y, cout, bad) == math.inf


def test_other_families_pass_clean_and_fail_defects():
    g = gen(41)
    # resample2x: nearest x2 up with prologue, 2x pool
    src = cl(2, (2, 4, 6), 40, 42)
    s, t = 1.0 + 0.2 * torch.randn(2, 64, generator=g), 0.3 * torch.randn(2, 64, generator=g)
    a = SH.silu(src.double() * s.double()[:, None, None, None] + t.double()[:, None, None, None])
    a[..., 40:] = 0
    up = a.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3).to(torch.bfloat16)
    assert SH.resample_ratio(src, 40, True, True, (s, t), True, up) <= 1.0
    up2 = up.clone()
    up2[:, :, 1::2] = up[:, :, ::2].roll(1, 2)
    assert SH.resample_ratio(src, 40, True, True, (s, t), True, up2) > 1.0
    pool = src.double().reshape(2, 2, 2, 2, 3, 2, 64).mean((3, 5)).to(torch.bfloat16)
    assert SH.resample_ratio(src, 40, False, False, None, False, pool) <= 1.0
    # linear_f32
    x, W, b = torch.randn(3, 64, generator=g), torch.randn(20, 64, generator=g), torch.randn(20, generator=g)
    y = (SH.silu(x.double()) @ W.double().t() + b.double()).float()
    assert SH.linear_ratio(x, W, b, True, y) <= 1.0
    assert SH.linear_ratio(x, W, b, False, y) > 1.0
    # layernorm / geglu
    h = torch.randn(5, 64, generator=g).to(torch.bfloat16)
    gm, bt = 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
    ln = F.layer_norm(h.double(), (64,), gm.double(), bt.double(), 1e-5).to(torch.bfloat16)
    assert SH.layernorm_ratio(h, gm, bt, 1e-5, ln) <= 1.0
    assert SH.layernorm_ratio(h, gm, bt, 1e-5, ln.roll(1, 0)) > 1.0
    gg = (h.double()[:, :32] * SH.gelu(h.double()[:, 32:])).to(torch.bfloat16)
    assert SH.geglu_ratio(h, 32, gg) <= 1.0
    assert SH.geglu_ratio(h, 32, (h.double()[:, 32:] * SH.gelu(h.double()[:, :32])).to(torch.bfloat16)) > 1.0
    _text_families(g)
    _patch_conv_family(g)
    _lpips_families(g)
    _interpolate_and_vq_families(g)


# ------------------------------------------------------------------------------------------------ text, 3-D, GAN and LPIPS families
def rnd(g, *shape):
    return torch.randn(*shape, generator=g)


def masked_sdpa(q, k, v, lens, scale):
    """[N, T, heads, hd] views -> scaled_dot_product_attention in fp64 under the key mask j < lens[n]."""
    T = k.shape[1]
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[:, None, None, :]
    return F.scaled_dot_product_attention(q.double().transpose(1, 2), k.double().transpose(1, 2), v.double().transpose(1, 2),
                                          attn_mask=mask, scale=scale).transpose(1, 2)


def test_attention_reference_with_key_lengths_equals_masked_sdpa():
    N, T, heads, hd = 3, 23, 2, 32
    g = gen(51)
    q, k, v = (rnd(g, N, T, heads, hd).to(torch.bfloat16) for _ in range(3))
    lens, scale = [5, 23, 1], hd ** -0.5
    want = masked_sdpa(q, k, v, lens, scale)
    for n in range(N):
        for h in range(heads):
            ref, _ = SH.attention_reference(q[n, :, h], k[n, :lens[n], h], v[n, :lens[n], h], scale)
            assert float((ref - want[n, :, h]).abs().max()) <= REF_TOL * float(want.abs().max())
    clean = want.to(torch.bfloat16)
    assert SH.attention_ratio(q, k, v, clean, scale, 0, lens) <= 1.0
    assert SH.attention_ratio(q, k, v, clean, scale, 0, [5, 99, 0]) <= 1.0           # the clamp: [1, Tkv]
    assert SH.attention_ratio(q, k, v, clean, scale, 0, None) > 1.0                 # judged against all Tkv keys: the old reference
    # planted: one sample's length off by one; two samples' lengths swapped
    assert SH.attention_ratio(q, k, v, masked_sdpa(q, k, v, [5, 22, 1], scale).to(torch.bfloat16), scale, 0, lens) > 1.0
    assert SH.attention_ratio(q, k, v, masked_sdpa(q, k, v, [6, 23, 1], scale).to(torch.bfloat16), scale, 0, lens) > 1.0
    assert SH.attention_ratio(q, k, v, masked_sdpa(q, k, v, [23, 5, 1], scale).to(torch.bfloat16), scale, 0, lens) > 1.0


def padded(t, cp):
    out = torch.zeros(tuple(t.shape[:-1]) + (cp,), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def _text_families(g):
    # gelu
    x = (3.0 * rnd(g, 7, 64)).to(torch.bfloat16)
    assert float((SH.gelu(x.double()) - F.gelu(x.double())).abs().max()) <= REF_TOL
    assert SH.gelu_ratio(x, F.gelu(x.double()).to(torch.bfloat16)) <= 1.0
    assert SH.gelu_ratio(x, F.gelu(x.double(), approximate="tanh").to(torch.bfloat16).roll(1, 1)) > 1.0
    assert SH.add_ratio(x, x.roll(1, 0), (x.double() + x.roll(1, 0).double()).to(torch.bfloat16)) <= 1.0
    assert SH.add_ratio(x, x.roll(1, 0), (x.double() + x.double()).to(torch.bfloat16)) > 1.0
    # layernorm_rows: C = 48 in rows of 64
    C, cp = 48, 64
    xr = padded((2.0 * rnd(g, 5, 1, 1, 3, C) + 0.5).to(torch.bfloat16), cp)
    gm, bt = 1 + 0.1 * rnd(g, C), 0.1 * rnd(g, C)
    ln = lambda t, width, w, b: F.layer_norm(t[..., :width].double(), (width,), w, b, 1e-5)
    ref, _ = SH.layernorm_reference(xr[..., :C].reshape(-1, C).double(), gm, bt, 1e-5)
    assert float((ref - ln(xr, C, gm.double(), bt.double()).reshape(-1, C)).abs().max()) <= REF_TOL * 10
    clean = padded(ln(xr, C, gm.double(), bt.double()).to(torch.bfloat16), cp)
    assert SH.layernorm_rows_ratio(xr, C, gm, bt, 1e-5, clean) <= 1.0
    over_cpad = padded((ln(xr, cp, None, None)[..., :C] * gm.double() + bt.double()).to(torch.bfloat16), cp)      # statistics over Cpad
    assert SH.layernorm_rows_ratio(xr, C, gm, bt, 1e-5, over_cpad) > 1.0
    dirty = clean.clone()
    dirty[2, 0, 0, 1, C + 3] = 2.0 ** -20                           # a non-zero pad lane
    assert SH.layernorm_rows_ratio(xr, C, gm, bt, 1e-5, dirty) == math.inf
    # embed_rows
    V, P, D, B, T = 97, 20, 48, 3, 7
    tok, pos = rnd(g, V, D), rnd(g, P, D)
    ids = torch.randint(0, V, (B, T), generator=g)
    want = F.embedding(ids, tok) + pos[:T][None]
    assert SH.embed_rows_ratio(ids, tok, pos, want) == 0.0 and SH.embed_rows_ratio(ids, tok, None, F.embedding(ids, tok)) == 0.0
    rows = lambda t: padded(t.to(torch.bfloat16), 64).reshape(B, 1, 1, T, 64)
    assert SH.embed_rows_ratio(ids, tok, pos, rows(want)) == 0.0
    shifted = F.embedding(ids, tok) + pos[1:T + 1][None]            # a position row shifted by one
    assert SH.embed_rows_ratio(ids, tok, pos, shifted) == math.inf and SH.embed_rows_ratio(ids, tok, pos, rows(shifted)) == math.inf
    dirty = rows(want).clone()
    dirty[1, 0, 0, 2, D] = 1.0
    assert SH.embed_rows_ratio(ids, tok, pos, dirty) == math.inf
    assert SH.embed_rows_ratio(ids, tok, pos, (want.double() * (1 + 2.0 ** -22)).float()) == math.inf       # bit-equal, not close
    # bert_embed
    typ = rnd(g, 2, D)
    tts = torch.randint(0, 2, (B, T), generator=g)
    tts[0, 0], tts[0, 1] = 1, 0
    emb = lambda tt: F.layer_norm((F.embedding(ids, tok) + F.embedding(tt, typ) + pos[:T][None]).double(), (D,), gm.double(), bt.double(), 1e-12)
    assert SH.bert_embed_ratio(ids, tts, tok, pos, typ, gm, bt, 1e-12, rows(emb(tts))) <= 1.0
    assert SH.bert_embed_ratio(ids, None, tok, pos, typ, gm, bt, 1e-12, rows(emb(torch.zeros_like(tts)))) <= 1.0
    assert SH.bert_embed_ratio(ids, tts, tok, pos, typ, gm, bt, 1e-12, rows(emb(torch.zeros_like(tts)))) > 1.0      # the token-type row ignored
    x32 = (F.embedding(ids, tok) + F.embedding(tts, typ)) + pos[:T][None]                                        # the kernel's fp32 sums
    assert SH.bert_embed_ratio(ids, tts, tok, pos, typ, gm, bt, 1e-12, rows(F.layer_norm(x32.double(), (D,), gm.double(), bt.double(), 1e-12))) <= 1.0


def torch_patch_conv(src, w, alpha, beta, kd, stride, slope, pad=2):
    """F.conv2d / conv3d(kernel 4) + affine + leaky_relu in fp64, channels-last [N, Do, Ho, Wo, Cout]; pad = 2 is the operation, pad = 1
    the planted defect at the same output extent (taps start at o * stride - 1)."""
    x = ncdhw(src)
    cout, cin = w.shape[0], src.shape[-1]
    Wf = torch.zeros((cout, cin, w.shape[2]), dtype=torch.float64)
    Wf[:, :w.shape[1]] = w.to(torch.bfloat16).double()
    lo, hi = pad, 4 - pad
    if kd == 1:
        y = F.conv2d(F.pad(x[:, :, 0], (lo, hi, lo, hi)), Wf.reshape(cout, cin, 4, 4), stride=stride)[:, :, None]
    else:
        y = F.conv3d(F.pad(x, (lo, hi, lo, hi, lo, hi)), Wf.reshape(cout, cin, 4, 4, 4), stride=stride)
    y = y.permute(0, 2, 3, 4, 1)
    y = y * (alpha[:cout].double() if alpha is not None else 1.0) + beta[:cout].double()
    return F.leaky_relu(y, slope)


@pytest.mark.parametrize("kd, stride", [(1, 1), (1, 2), (4, 1), (4, 2)])
def test_patch_conv_reference_equals_torch_conv(kd, stride):
    g = gen(60 + kd + stride)
    sp = (1, 9, 10) if kd == 1 else (3, 5, 6)
    src = cl(2, sp, 24, 61, cpad=32)
    cout = 40
    w = rnd(g, cout, 24, 16 * kd) * 0.1
    alpha, beta = padded(1 + 0.3 * rnd(g, cout), 64), padded(0.5 * rnd(g, cout), 64)
    want = torch_patch_conv(src, w, alpha, beta, kd, stride, 0.2)
    same = F.conv2d(ncdhw(src)[:, :, 0], torch.zeros(1, 32, 4, 4, dtype=torch.float64), stride=stride, padding=2) if kd == 1 else \
        F.conv3d(ncdhw(src), torch.zeros(1, 32, 4, 4, 4, dtype=torch.float64), stride=stride, padding=2)
    assert tuple(want.shape[1:4]) == SH.patch_conv_extent(sp, kd, stride) == ((1,) if kd == 1 else ()) + tuple(same.shape[2:])
    pos = SH._all_positions(want.shape[1:4])
    for n in range(2):
        ref, bound = SH.patch_conv_reference(src, w, alpha, beta, kd, stride, 0.2, n, pos)
        assert float((ref - want[n][pos[:, 0], pos[:, 1], pos[:, 2]]).abs().max()) <= REF_TOL * float(want.abs().max())
        assert bool((bound > 0).all())


def _patch_conv_family(g):
    for kd, stride, dtype, with_alpha in ((1, 2, torch.bfloat16, True), (4, 1, torch.bfloat16, True), (1, 1, torch.float32, False)):
        sp = (1, 9, 10) if kd == 1 else (3, 5, 6)
        src = cl(2, sp, 24, 62, cpad=32)
        cout = 40
        w = rnd(g, cout, 24, 16 * kd) * 0.1
        alpha = padded(1 + 0.3 * rnd(g, cout), 64) if with_alpha else None
        beta = padded(0.5 * rnd(g, cout), 64)
        out = lambda y: padded(y.to(dtype), 64)
        ratio = lambda got: SH.patch_conv_ratio(src, w, alpha, beta, cout, kd, stride, 0.2, got)
        clean = out(torch_patch_conv(src, w, alpha, beta, kd, stride, 0.2))
        assert ratio(clean)[1] == 2 and ratio(clean)[0] <= 1.0
        assert ratio(out(torch_patch_conv(src, w, alpha, beta, kd, stride, 0.2, pad=1)))[0] > 1.0               # padding 1
        if with_alpha:
            sw = list(range(64))
            sw[3], sw[4] = 4, 3
            assert ratio(out(torch_patch_conv(src, w, alpha[sw], beta[sw], kd, stride, 0.2)))[0] > 1.0           # alpha / beta of two channels swapped
        short = clean.clone()
        short[:, :, -1] = 0                                                                                    # the last output row missing
        assert ratio(short)[0] > 1.0
        dirty = clean.clone()
        dirty[1, 0, 0, 0, cout] = 2.0 ** -20
        assert ratio(dirty)[0] == math.inf
        assert ratio(clean[:, :, :-1])[0] == math.inf                                                          # a wrong extent


def _lpips_families(g):
    import lpips_ref
    # relu, pooled halves, tap value
    a = rnd(g, 3, 1, 5, 7, 64).to(torch.bfloat16)
    b = (a.float() + 0.5 * rnd(g, 3, 1, 5, 7, 64)).to(torch.bfloat16)
    lw = torch.rand(64, generator=g) + 0.05
    assert SH.relu_ratio(a, F.relu(a)) == 0.0 and SH.relu_ratio(a, a.abs()) == math.inf
    pool = lambda t: F.max_pool2d(F.relu(t[:, 0].permute(0, 3, 1, 2).float()), 2).permute(0, 2, 3, 1).to(t.dtype)[:, None]
    pooled = torch.cat([pool(a), pool(b)])
    assert torch.equal(SH.lpips_pool_reference(a, b), pooled)
    nchw = lambda t: F.relu(t.double())[:, 0].permute(0, 3, 1, 2)
    want = lpips_ref.tap_distance(nchw(a), nchw(b), lw.double())
    assert float((SH.lpips_tap_reference(a, b, lw) - want).abs().max()) <= REF_TOL
    got = want.float()
    assert SH.lpips_tap_ratio(a, b, lw, got, pooled, got.clone(), None) <= 1.0
    before = torch.full((3,), 2.0)
    assert SH.lpips_tap_ratio(a, b, lw, got, pooled, before + got, before) <= 1.0
    assert SH.lpips_tap_ratio(a, b, lw, got, pooled, before, before) == math.inf                               # total not updated
    assert SH.lpips_tap_ratio(a, b, lw, got, torch.cat([pool(b), pool(a)])) == math.inf                        # a's and b's halves swapped
    assert SH.lpips_tap_ratio(a, b, lw, (want * (1 + 4 * SH.LPIPS_TAP_RTOL)).float()) > 1.0
    assert SH.lpips_tap_ratio(a, b, lw, got.flip(0)) > 1.0
    # volume views: the reference's rearrange and ScalingLayer
    x = torch.rand(2, 4, 5, 6, generator=g) * 1.5 - 0.25
    shift, scale = torch.tensor(lpips_ref.SHIFT), torch.tensor(lpips_ref.SCALE)
    for view in range(3):
        imgs = lpips_ref.views(x[:, None].double())[view]
        want = lpips_ref.scaling(imgs).permute(0, 2, 3, 1)
        n0, n1 = 1, imgs.shape[0] - 2
        ref, _ = SH.volume_views_reference(x, view, n0, n1, shift, scale)
        assert float((ref - want[n0:n1]).abs().max()) <= 1e-6                                  # scaling() holds shift / scale in fp32
        for dtype in (torch.float32, torch.bfloat16):
            clean = padded(ref.to(dtype), 32)[:, None]
            assert SH.volume_views_ratio(x, view, n0, n1, shift, scale, clean) <= 1.0
            assert SH.volume_views_ratio(x, (view + 1) % 3, n0, n1, shift, scale, clean) > 1.0          # another axis (another extent: inf)
            assert SH.volume_views_ratio(x, view, n0 - 1, n1 - 1, shift, scale, clean) > 1.0            # the image range off by one
            dirty = clean.clone()
            dirty[0, 0, 0, 0, 3] = 1.0
            assert SH.volume_views_ratio(x, view, n0, n1, shift, scale, dirty) == math.inf
    x3 = torch.rand(3, 3, 5, 7, generator=g)
    ref, _ = SH.volume_views_reference(x3, 3, 1, 3, shift, scale)
    assert float((ref - lpips_ref.scaling(x3.double()).permute(0, 2, 3, 1)[1:3]).abs().max()) <= 1e-6


MODES = ("nearest", "bilinear", "bicubic", "area")


@pytest.mark.parametrize("mode", MODES)
def test_interpolate_reference_equals_f_interpolate(mode):
    g = gen(70)
    for shape in ((2, 3, 17, 20), (1, 2, 13, 10), (1, 1, 2, 3)):
        x = rnd(g, *shape)
        for s in (0.5, 2):
            ref, mag = SH.interpolate2d_reference(x, s, mode)
            want = F.interpolate(x.double(), scale_factor=s, mode=mode)
            assert ref.shape == want.shape and float((ref - want).abs().max()) <= REF_TOL * 100, (shape, s)
            assert bool((mag >= ref.abs() - 1e-12).all())
            assert SH.interpolate2d_ratio(x, s, mode, want.float()) <= 1.0
            assert want.shape[3] == 1 or SH.interpolate2d_ratio(x, s, mode, want.float().roll(1, 3)) > 1.0


def _interpolate_and_vq_families(g):
    # bilinear at scale 0.5 without the half-pixel offset: source 2 d instead of 2 d + 0.5
    x = rnd(g, 2, 3, 16, 20)
    assert SH.interpolate2d_ratio(x, 0.5, "bilinear", F.interpolate(x, scale_factor=0.5, mode="bilinear")) <= 1.0
    assert SH.interpolate2d_ratio(x, 0.5, "bilinear", x[:, :, ::2, ::2].contiguous()) > 1.0
    assert SH.interpolate2d_ratio(x, 0.5, "bilinear", F.interpolate(x, scale_factor=0.5, mode="bilinear")[:, :, :-1]) == math.inf
    # vq_nearest
    E = rnd(g, 16, 4)
    z = padded(rnd(g, 200, 4), 8)
    idx, second, tie = SH.vq_reference(z[:, :4], E)
    assert torch.equal(idx, torch.cdist(z[:, :4].double(), E.double()).argmin(1)) and float(tie.double().mean()) <= SH.VQ_TIE_CAP
    st = lambda i: z[:, :4] + (E[i] - z[:, :4])
    assert SH.vq_ratio(z, E, idx.int(), st(idx)) == (0.0, float(tie.double().mean()))
    m = int((~tie).nonzero()[0])
    bad = idx.clone()
    bad[m] = second[m]                                              # one row given the second-nearest code, outside the margin
    assert SH.vq_ratio(z, E, bad.int(), st(bad))[0] == math.inf
    assert SH.vq_ratio(z, E, idx.int(), E[idx])[0] == math.inf       # the codebook row itself is not the straight-through expression
    dE = torch.cdist(E.double(), E.double()) + 1e9 * torch.eye(16, dtype=torch.float64)
    ci, cj = divmod(int(dE.argmin()), 16)                           # the closest pair of codes: their midpoint is nearest to exactly these two
    zt = z.clone()
    zt[0, :4] = (E[ci] + E[cj]) / 2                                   # a row on the bisector of two codes: either may win, nothing else
    i2, s2, t2 = SH.vq_reference(zt[:, :4], E)
    assert bool(t2[0]) and {int(i2[0]), int(s2[0])} == {ci, cj}
    if True:
        for pick, ok in ((int(i2[0]), True), (int(s2[0]), True), ((int(i2[0]) + 1) % 16 if (int(i2[0]) + 1) % 16 != int(s2[0]) else (int(i2[0]) + 2) % 16, False)):
            alt = i2.clone()
            alt[0] = pick
            assert (SH.vq_ratio(zt, E, alt.int())[0] == 0.0) == ok
    many = z.clone()
    many[:10, :4] = ((E[ci] + E[cj]) / 2)[None]
    r, share = SH.vq_ratio(many, E, SH.vq_reference(many[:, :4], E)[0].int())                 # 10 of 200 rows on a bisector: over the cap
    assert share >= 0.05 > SH.VQ_TIE_CAP and r == math.inf


def test_vq_fixture_rows_stay_under_the_near_tie_cap():
    """The rows the 3-D VQ first stage quantises in tests/test_shadow_nets_gpu.py: the reference's recorded pre-quantisation rows of the
    fixture volume against the seeded codebook.  Their own fp64 near-tie share stays under VQ_TIE_CAP."""
    import json
    import os
    from util import GOLD, T, gold
    from jointimagegeneration_amd.synth import synth_tensor
    from test_ae3d_cpu import vq3d
    from util import seeded
    with open(os.path.join(GOLD, "ae3d_surface.json")) as f:
        meta = json.load(f)
    E = seeded(vq3d(meta), "ae3d_vq.").quantize.embedding.weight.detach() * meta["code_scale"]
    z = T(gold("ae3d")["vq_prequant"])
    rows = z.permute(0, 2, 3, 4, 1).reshape(-1, z.shape[1])
    idx, _, tie = SH.vq_reference(rows, E)
    assert torch.equal(idx, T(gold("ae3d")["vq_idx"]).long().reshape(-1))
    assert float(tie.double().mean()) <= SH.VQ_TIE_CAP, float(tie.double().mean())


# ------------------------------------------------------------------------------------------------ operand contract
def _cl(t, C):
    from jointimagegeneration_amd.ops import CL
    return CL(t, C)


def _conv_args(**over):
    a = dict(src1=_cl(cl(2, (1, 5, 6), 40, 80), 40), src2=None, weight=torch.zeros(8, dtype=torch.bfloat16), bias=torch.zeros(64), cout=48,
             k=(1, 3, 3), stride=1, pad=1, upsample=False, residual=None, bias_per_sample=False, prologue=None, prologue_acc=None, skip=None,
             out=None, ddim=None, geglu=False)
    a.update(over)
    return a


def _gn_args(**over):
    a = dict(src1=_cl(cl(2, (1, 5, 6), 64, 81), 64), src2=None, gamma=torch.ones(64), beta=torch.zeros(64), eps=1e-5)
    a.update(over)
    return a


def _attn_args(**over):
    qkv = torch.zeros(2, 1, 1, 7, 3 * 64, dtype=torch.bfloat16)
    a = dict(q=qkv, k=qkv, v=qkv, out=torch.zeros(2, 1, 1, 7, 64, dtype=torch.bfloat16), N=2, heads=2, head_dim=32, Tq=7, Tkv=7, ld_hs_q=(192, 32),
             ld_hs_k=(192, 32), ld_hs_v=(192, 32), ld_hs_o=(64, 32), q_off=0, k_off=64, v_off=128, kv_len=None)
    a.update(over)
    return a


def _contract_cases():
    bf, f32 = torch.bfloat16, torch.float32
    x = torch.zeros(4, 64, dtype=bf)
    lin = dict(x=torch.zeros(3, 16), W=torch.zeros(8, 16), b=torch.zeros(8), out=None)
    res_ok = _cl(cl(2, (1, 5, 6), 48, 82), 48)
    return [
        # (rule, op, clean arguments, violating arguments, operand named, word in what was found)
        ("dtype", "layernorm", dict(x=x, gamma=torch.ones(64), beta=torch.zeros(64)), dict(x=x, gamma=torch.ones(64, dtype=bf), beta=torch.zeros(64)), "gamma", "dtype"),
        ("contiguous", "conv", _conv_args(), _conv_args(src1=_cl(cl(2, (1, 5, 12), 40, 80)[:, :, :, ::2], 40)), "src1", "stride"),
        ("forwarded stride", "film_fold", dict(scale=torch.zeros(2, 128)[:, :96], shift=torch.zeros(2, 128)[:, :96], C=64),
         dict(scale=torch.zeros(2, 128)[:, :96], shift=torch.zeros(2, 96), C=64), "shift", "stride"),
        ("gamma / beta >= c_log", "groupnorm_stats", _gn_args(), _gn_args(gamma=torch.ones(32)), "gamma", "extent"),
        ("gamma / beta >= c_log", "groupnorm_fused", _gn_args(), _gn_args(beta=torch.zeros(63)), "beta", "extent"),
        ("scale / shift [N, C1 + C2]", "groupnorm_apply", dict(_gn_args(src2=_cl(cl(2, (1, 5, 6), 32, 83), 32)), scale=torch.zeros(2, 96), shift=torch.zeros(2, 96)),
         dict(_gn_args(src2=_cl(cl(2, (1, 5, 6), 32, 83), 32)), scale=torch.zeros(2, 96), shift=torch.zeros(2, 64)), "shift", "extent"),
        ("bias pad32(cout)", "conv", _conv_args(), _conv_args(bias=torch.zeros(48)), "bias", "extent"),
        ("bias per sample", "conv", _conv_args(bias=torch.zeros(128), bias_per_sample=True), _conv_args(bias=torch.zeros(64), bias_per_sample=True), "bias", "extent"),
        ("residual = output shape", "conv", _conv_args(residual=res_ok), _conv_args(residual=_cl(cl(2, (1, 5, 5), 48, 82), 48)), "residual", "extent"),
        ("prologue[1] matches prologue[0]", "resample2x", dict(src=_cl(cl(2, (2, 4, 6), 40, 84), 40), prologue=(torch.zeros(2, 64), torch.zeros(2, 64))),
         dict(src=_cl(cl(2, (2, 4, 6), 40, 84), 40), prologue=(torch.zeros(2, 64), torch.zeros(2, 40))), "prologue[1]", "extent"),
        ("add: equal numel", "add", dict(a=x, b=x.clone()), dict(a=x, b=x[:3].clone()), "b", "extent"),
        ("layernorm: contiguous bf16", "layernorm", dict(x=x, gamma=torch.ones(64), beta=torch.zeros(64)),
         dict(x=torch.zeros(4, 128, dtype=bf)[:, :64], gamma=torch.ones(64), beta=torch.zeros(64)), "x", "stride"),
        ("geglu: contiguous bf16", "geglu", dict(h=x, inner=32), dict(h=x.float(), inner=32), "h", "dtype"),
        ("linear_f32: W [O, I]", "linear_f32", lin, dict(lin, W=torch.zeros(8, 32)[:, :16]), "W", "stride"),
        ("linear_f32: W [O, I]", "linear_f32", lin, dict(lin, W=torch.zeros(8, 12)), "W", "extent"),
        ("linear_f32: b [O]", "linear_f32", lin, dict(lin, b=torch.zeros(4)), "b", "extent"),
        ("attention views inside their tensors", "attention", _attn_args(), _attn_args(v_off=129), "v", "extent"),
        ("attention views inside their tensors", "attention", _attn_args(kv_len=torch.ones(2, dtype=torch.int32)), _attn_args(kv_len=torch.ones(2, dtype=torch.int64)), "kv_len", "dtype"),
        ("ddim_step rows", "ddim_step", dict(x=torch.zeros(6, 4), eps=torch.zeros(6, 32), scalars=torch.zeros(4), noise=None, pred_x0_out=None, unet_in=None),
         dict(x=torch.zeros(6, 4), eps=torch.zeros(5, 32), scalars=torch.zeros(4), noise=None, pred_x0_out=None, unet_in=None), "eps", "extent"),
    ]


@pytest.mark.parametrize("case", _contract_cases(), ids=lambda c: f"{c[1]}-{c[0]}".replace(" ", "_"))
def test_contract_violations_are_named(case):
    rule, op, clean, bad, operand, word = case
    assert SH.contract_violations(op, clean, None) == [], rule
    found = SH.contract_violations(op, bad, None)
    assert [o for o, _ in found] == [operand] and word in found[0][1], (rule, found)
    # the device rule: host tensors handed to a kernel that reads device memory, every tensor operand named
    on_host = SH.contract_violations(op, clean, "cuda")
    assert on_host and all("device" in what for _, what in on_host), on_host


def test_contract_record_fails_assert_within_bounds():
    """What the harness does with a violation: a `contract` record with ratio inf that assert_within_bounds reports by op and operand."""
    sh = SH.Shadow.__new__(SH.Shadow)
    sh.records, sh.calls = [], 0
    import inspect
    sh.sig = {"add": inspect.signature(lambda a, b: None)}
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    sh._args("add", (x, x[:3].clone()), {})
    assert [r.family for r in sh.records] == ["contract", "contract", "contract"]          # two host tensors and the short operand
    assert all(r.ratio == math.inf for r in sh.records) and dict(sh.records[-1].plan)["operand"] == "b"
    with pytest.raises(AssertionError, match=r"contract.*'op': 'add'.*'operand': 'b'"):
        sh.assert_within_bounds(1)


# ------------------------------------------------------------------------------------------------ completeness
NETWORK_MODULES = ("cond", "lpips", "aeloss", "blocks", "unet", "ldm", "chain")


def ops_calls(source: str):
    """every X of an `ops.X(...)` call in `source`"""
    import ast
    return {n.func.attr for n in ast.walk(ast.parse(source))
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and isinstance(n.func.value, ast.Name) and n.func.value.id == "ops"}


def undecided(names):
    return sorted(n for n in names if n not in SH.WRAPPED and n not in SH.EXEMPT)


def test_every_ops_call_of_the_network_modules_is_wrapped_or_exempt():
    import os
    import jointimagegeneration_amd as pkg
    from jointimagegeneration_amd import ops
    called = set()
    for mod in NETWORK_MODULES:
        with open(os.path.join(os.path.dirname(pkg.__file__), mod + ".py")) as f:
            names = ops_calls(f.read())
        assert names, mod
        called |= names
    assert {"conv", "attention", "patch_conv", "lpips_tap", "vq_nearest", "bert_embed", "to_cl"} <= called       # the walk does find calls
    assert undecided(called) == [], f"ops calls of the network modules that tests/shadow.py neither wraps nor exempts: {undecided(called)}"
    assert not set(SH.WRAPPED) & set(SH.EXEMPT)
    assert all(hasattr(ops, n) for n in list(SH.WRAPPED) + list(SH.EXEMPT)) and all(len(r) > 8 and "\n" not in r for r in SH.EXEMPT.values())
    assert undecided(ops_calls("y = ops.conv(x)\nz = ops.brand_new_kernel(y, 1)\n")) == ["brand_new_kernel"]     # a new op fails by name
    assert "to_cl" in SH.EXEMPT and undecided(called | {"to_cl_v2"}) == ["to_cl_v2"]
