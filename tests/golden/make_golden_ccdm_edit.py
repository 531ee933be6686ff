"""Generates tests/golden/ccdm_edit.npz from the REFERENCE on CPU: the two forward-noising draws that CCDM mask editing runs on.

For K in {2, 14, 16, 17, 32}, the cosine schedule of T = 50 and one sample of 4x4x4 voxels per t in (1, 2, 25, 50):
`q_xt_given_x0(onehot(known), t).sample()` and `q_xt_given_xtm1(onehot(known), t).sample()`
(ccdm/ddpm/models/diffusion_denoising.py:73-89, one_hot_categorical.py) as labels under a seed, and the exponential tape that is the same
draw from a generator of that seed (`sample()` equals argmax p / E bit for bit; as make_golden_losses.py's `draw`).  Stored per
(K, distribution): the seed, the known labels, the drawn labels, the tape [256, K] and the mix rows (keep, unif) [4, 2] as the reference
forms them; per K the schedule rows betas / cumalphas.  Nothing else.

Every stored race is asserted to be decided: the two best quotients of a row differ by more than 2^-20 relatively (fp64 restatement,
tests/losses_ref.race), so the fixture alone decides every label, and tests/ccdm_edit_ref.py is asserted to reproduce the labels.

Run only in the build container (needs the reference tree, like make_golden.py):
    python tests/golden/make_golden_ccdm_edit.py [OUT_DIR]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
import ccdm_edit_ref as ER  # noqa: E402
import losses_ref as R  # noqa: E402

torch.set_grad_enabled(False)


def draw(oh, probs_bchw, seed, M, K):
    """The reference's .sample() under a seed, and the exponential tape that is the same draw."""
    torch.manual_seed(seed)
    lab = oh.OneHotCategoricalBCHW(probs=probs_bchw).sample().argmax(dim=1)
    return lab, torch.empty(M, K).exponential_(1, generator=MG.g(seed))


def main(out_dir):
    dd, oh, *_ = MG.import_ccdm()
    out = {}
    S = int(np.prod(ER.FX_SP))
    N = len(ER.TS)
    t = torch.tensor(ER.TS)
    for K in ER.KS:
        dmod = dd.DiffusionModel("cosine", ER.T_STEPS, K, dims=3)
        known = torch.randint(0, K, (N,) + ER.FX_SP, generator=MG.g(5000 + K))
        x0 = MG.S.one_hot_bchw(known, K)
        out[f"k{K}_known"] = known.int()
        out[f"k{K}_betas"], out[f"k{K}_cumalphas"] = dmod.betas.clone(), dmod.cumalphas.clone()
        for name, fn, mix, seed in (("qx0", dmod.q_xt_given_x0, torch.stack([dmod.cumalphas[t - 1], 1 - dmod.cumalphas[t - 1]], 1), 6000 + K),
                                    ("qxtm1", dmod.q_xt_given_xtm1, torch.stack([1 - dmod.betas[t - 1], dmod.betas[t - 1]], 1), 7000 + K)):
            dist = fn(x0, t)
            lab, E = draw(oh, dist.probs.permute(0, 4, 1, 2, 3), seed, N * S, K)
            mine, gap = R.race(R.keep_probs(known.numpy(), mix[:, 0], mix[:, 1], K), E)
            assert np.array_equal(mine, R.rows(lab.numpy())), f"K={K} {name}: the fp64 race disagrees with the reference's draw"
            assert float(gap.min()) > R.GAP_MIN, f"K={K} {name}: an undecidable race in the fixture (gap {gap.min():.3e})"
            rest = ER.q_sample(known.view(-1), mix, S, K, E)
            assert torch.equal(rest, lab.view(-1).int()), f"K={K} {name}: the fp32 restatement disagrees with the reference's draw"
            print(f"  K={K:2d} {name}: {N * S} races, smallest gap {gap.min():.3e}")
            out.update({f"k{K}_{name}_seed": np.asarray(seed), f"k{K}_{name}_labels": lab.int(), f"k{K}_{name}_E": E,
                        f"k{K}_{name}_mix": mix.float().clone()})
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "ccdm_edit.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.OUT)
