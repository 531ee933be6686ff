"""CPU suite: the shadow harness (tests/shadow.py) itself.  Its fp64 references equal torch's CPU operators (F.conv2d / conv3d,
F.group_norm, scaled-dot-product attention, in fp64) to 1e-12 on small shapes with every conv feature production uses, and its
comparator passes a clean kernel-like output (the reference rounded to the kernel's output type) but fails on each injected defect."""
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
