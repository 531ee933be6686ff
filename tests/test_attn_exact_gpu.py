"""GPU suite (-m gpu): every path of the flash-attention kernel bit for bit against the fp64 reference rounded to bf16, on inputs where
every fp32 operation of the kernel is exact (tests/attn_exact.py: the regimes, their preconditions, the comparators, the packer).
The exact tests have no tolerance.

Paths, each proven by gg_attention_plan on the shape of the launch itself (attn_exact.assert_path: a shape that no longer reaches the
path it is named for fails):
  plain    attn_kernel<D, KT>, register-staged K/V tiles (D < 256)
  ws2      attn_kernel<D, KT, 2>: the keys split over the two wave groups of a workgroup, merged through LDS
  dma      D >= 256: K/V tiles double-buffered in LDS by LDS-DMA with a hand-counted s_waitcnt
  split    dma + the keys split over workgroups, attn_merge_kernel as a second launch; every such case runs a second time through the
           raw descriptor WITHOUT a workspace (the unsplit fallback), and the two results must be bit-identical
Every case runs in the sel, grp and uni regimes; the layouts (legacy head-major q|k|v, new order, q separate from packed k|v with
Tq != Tkv, the autoencoder's single head with a padded leading dimension) are spread over the cases of every path.  Every element of
the q / k / v buffers outside the addressed (token, head, d) slots is NaN, the output buffer has ldo > heads * D, three rows beyond
N * Tq and a sentinel everywhere: a stray read poisons the result, a stray write is counted.

Two hardware facts underlie the exact regimes: v_exp_f32(0) == 1.0 and v_exp_f32(x <= -500) == 0.  The regimes themselves are the
measurement: were either false, every sel / grp case would differ from the closed form.  Measured on an MI355X: every case of every
path is bit exact in all three regimes, so both facts hold.

The peaked leg (attn_exact.peaked) is held to shadow.attention_ratio <= 1 with the shadow harness's bound and prints its worst ratio.

gg_attention_forward_f32 (D <= 64) multiplies q and k by sqrt(scale) each; with scale = 2^-4 that is exact and the three regimes hold
for it with the same expected values (fp32 storage).  Measured: its expf keeps all three regimes, grp included, bit exact.
"""
import pytest
import torch

import attn_exact as X

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def prepared(case, regime, dev, dtype=torch.bfloat16, scale=None):
    """(inputs, packed device buffers) of a case; the fp64 reference is computed on the device and compared with the closed form once"""
    key = (case.name, regime)
    if key not in _CACHE:
        inp = X.build(case, regime, dtype=dtype, scale=scale)
        X.check_reference(regime, inp, X.reference(inp, dev))
        _CACHE[key] = (inp, X.pack(case, inp).to(dev))
    return _CACHE[key]


def run(case, p, scale, workspace=True):
    """one launch into a fresh sentinel-filled copy of the output buffer"""
    q = X.Packed(p.q, p.k, p.v, p.out.clone(), p.ld_hs_q, p.ld_hs_k, p.ld_hs_v, p.ld_hs_o, p.q_off, p.k_off, p.v_off)
    X.launch(case, q, scale, workspace)
    torch.cuda.synchronize()
    return q.out


PAIRS = [pytest.param(c, r, id=f"{c.name}-{r}") for c in X.CASES for r in c.regimes()]


@pytest.mark.parametrize("case,regime", PAIRS)
def test_attention_bit_exact(case, regime, dev):
    X.assert_path(case)
    inp, p = prepared(case, regime, dev)
    out = run(case, p, inp.scale)
    bad = X.check_output(case, inp, out)
    assert not bad, f"{case.name} [{regime}] plan {case.plan}: {bad}"
    if case.ks > 1:
        out1 = run(case, p, inp.scale, workspace=False)
        bad = X.check_output(case, inp, out1)
        assert not bad, f"{case.name} [{regime}] without a workspace: {bad}"
        assert not X.mismatches(X.out_view(case, out1), X.out_view(case, out))


@pytest.mark.parametrize("name", X.PEAKED)
def test_attention_peaked_within_the_shadow_bound(name, dev):
    case = X.CASE[name]
    X.assert_path(case)
    inp = X.peaked(case)
    p = X.pack(case, inp).to(dev)
    for workspace in ((True, False) if case.ks > 1 else (True,)):
        out = run(case, p, inp.scale, workspace)
        assert X.stray_writes(case, out) == 0
        ratio = X.peaked_ratio(case, inp, out)
        print(f"peaked {case.path}{'' if workspace else ' (no workspace)'} {name}: worst shadow ratio {ratio:.3f}")
        assert ratio <= 1.0, (name, workspace, ratio)


@pytest.mark.parametrize("case", X.F32_CASES, ids=lambda c: c.name)
def test_attention_f32_bit_exact(case, dev):
    for regime in case.regimes():
        inp, p = prepared(case, regime, dev, dtype=torch.float32, scale=X.F32_SCALE)
        out = run(case, p, inp.scale)
        bad = X.check_output(case, inp, out)
        assert not bad, f"{case.name} [{regime}]: {bad}"
