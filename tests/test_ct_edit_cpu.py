"""CPU suite: the reference of the CT editing loop (tests/ct_edit_ref.py) against the oracle's un-edited loop, its window rule against
max_pool2d, and the visit list against the pipeline's slice window."""
import pytest
import torch
import torch.nn.functional as F

import ct_edit_ref as R
from util import sd_cpu, small_ldm, synth_labels

torch.set_grad_enabled(False)


def _labels(lo, hi, Dm=5, HW=32, seed=2):
    lab = torch.zeros((Dm, HW, HW), dtype=torch.int64)
    lab[lo:hi] = torch.from_numpy(synth_labels((hi - lo, HW, HW), 12, seed=seed))
    lab[lo:hi, 2:5, 2:5] = 7
    return lab


@pytest.fixture(scope="module")
def model():
    m = small_ldm()
    return sd_cpu(m), m.alphas_cumprod.cpu()


def test_reference_with_nothing_kept_is_the_oracle_slice_loop(model):
    from util import oracle_slice_loop
    sd, ac = model
    steps = 4
    lab = _labels(1, 3)                                                    # window m = 0 .. 2
    whole = (lab.float() / 255.0)[None, None]
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(3)]
    want = oracle_slice_loop(sd, whole, xs, steps, ac, 32)
    known = torch.rand(lab.shape, generator=g)
    got = R.edited_slices_on_state_dict(sd, whole, known, torch.zeros(lab.shape, dtype=torch.bool), xs, [], steps, ac, 32, f=4, r=1)
    assert torch.equal(got, want)
    assert float(got[0, 0, 1].abs().max()) > 0 and float(got[0, 0, 4].abs().max()) == 0


def test_reference_with_everything_kept_returns_known_and_calls_no_network():
    calls = []

    def stub(name):
        def fn(*a):
            calls.append(name)
            raise AssertionError(f"{name} was called")
        return fn

    lab = _labels(0, 5)
    whole = (lab.float() / 255.0)[None, None]
    known = torch.rand(lab.shape, generator=torch.Generator().manual_seed(1))
    got = R.edited_slices(stub("cond_encode"), stub("first_stage_encode"), stub("eps_model_for"), stub("decode"), whole, known,
                          torch.ones(lab.shape, dtype=torch.bool), [], [], torch.linspace(0.999, 0.01, 1000), 3, 4, 0)
    assert calls == [] and torch.equal(got[0, 0], known)


# every (f, hw, r) whose window f (2 r + 1) fits the image (a wider one is refused on the host); (2, 6, 1) and (8, 40, 2): the window IS the image
@pytest.mark.parametrize("f,hw,r", [(4, 32, 0), (4, 32, 1), (4, 32, 2), (8, 16, 0), (8, 48, 1), (8, 40, 2), (2, 6, 0), (2, 6, 1)])
def test_window_rule_is_max_pool_of_the_unkept_pixels(f, hw, r):
    g = torch.Generator().manual_seed(100 * f + r)
    cases = [torch.ones(hw, hw, dtype=torch.bool), torch.zeros(hw, hw, dtype=torch.bool), torch.rand(hw, hw, generator=g) > 0.02]
    for y, x in ((0, 0), (0, hw - 1), (hw - 1, 0), (hw - 1, hw - 1), (f - 1, f), (f, f - 1), (f, f), (hw // 2, hw // 2 - 1)):
        k = torch.ones(hw, hw, dtype=torch.bool)
        k[y, x] = False                                                    # corners (windows that leave the image), cell boundaries
        cases.append(k)
    for k in cases:
        want = 1.0 - F.max_pool2d((~k).float()[None, None], kernel_size=f * (2 * r + 1), stride=f, padding=r * f)[0, 0]
        assert torch.equal(R.latent_keep_mask(k, f, r), want)
    one = R.latent_keep_mask(cases[3], f, r)                               # pixel (0, 0) un-kept: exactly the cells within r of cell (0, 0)
    assert int((one == 0).sum()) == min(r + 1, hw // f) ** 2


def test_visit_list_skips_kept_slices_wraps_and_can_be_empty():
    from jointimagegeneration_amd.pipeline import slice_window
    depth = 7
    lab = _labels(0, 3, Dm=5, HW=16).int()                                 # non-empty on slice 0: the window starts at m = -1
    win = slice_window(lab, depth)
    assert win[0] == -1 and win == list(range(-1, win[-1] + 1)) and len(win) >= 4
    keep = torch.zeros((depth, 8, 8), dtype=torch.bool)
    assert R.visit_list(win, keep) == (win, [False] * len(win))
    keep[1] = True                                                         # a fully kept slice is skipped
    keep[2, 0, 0] = True                                                   # one kept pixel: mixed
    keep[depth - 1, :, :4] = True                                          # the wrap-around slice m = -1 is slice depth - 1: mixed
    visit, mixed = R.visit_list(win, keep)
    assert visit == [m for m in win if m != 1]
    assert mixed == [m in (-1, 2) for m in visit]
    keep[:] = True
    keep[depth - 2] = False                                                # un-kept, but outside the window: not visited
    assert depth - 2 not in [m % depth for m in win]
    assert R.visit_list(win, keep) == ([], [])
