"""CPU suite: the integer restatement of the CCDM Philox draw (philox_ref.py) against the published known answers, and the proof that the
inputs test_sampler_exact_gpu.py compares are sensitive to each defect the draw could have and still mix, repeat and match itself."""
import numpy as np
import pytest

import philox_ref as P

# Random123 known answers of philox4x32-10 (kat_vectors): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("kat", KAT, ids=["zero", "ones", "pi"])
def test_philox4x32_10_known_answers(kat):
    ctr, key, want = kat
    got = tuple(int(v) for v in P.philox4x32_10(ctr, key))
    assert got == want, [hex(v) for v in got]


def test_counter_layout_of_the_reference_draw():
    """Row 0 of seed 0 at offset 0 is the all-zero known answer; every other word is the block of its own (row, q4, offset, key)."""
    w = P.draw_words(5, 32)
    assert tuple(int(v) for v in w[0, :4]) == KAT[0][2]
    seed, off, row, q4 = P.SEED_HI, 2 ** 32 + 7, 1300, 5
    w = P.draw_words(3 * P.ROWS_PER_SAMPLE, 32, seeds=(1, seed, 2), rows_per_sample=P.ROWS_PER_SAMPLE, offset=off)
    blk = P.philox4x32_10((row, 0, q4, 7), (seed & 0xFFFFFFFF, seed >> 32))
    assert [int(v) for v in w[P.ROWS_PER_SAMPLE + row, 4 * q4:4 * q4 + 4]] == [int(v) for v in blk]
    assert np.array_equal(P.draw_words(64, 16), P.draw_words(64, 32)[:, :16])            # K <= 16 and K > 16 agree on the first 16 classes
    assert np.array_equal(P.draw_words(64, 16, offset=2 ** 32 + 7), P.draw_words(64, 16, offset=7))
    assert not np.array_equal(P.draw_words(64, 16, offset=7), P.draw_words(64, 16))


def test_word_to_uniform_map_is_exact_and_in_range():
    w = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32)
    u = P.words_to_u(w)
    assert u.dtype == np.float32
    assert [float(v) for v in u] == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.0]
    assert float(P.exp_ref(w)[-1]) == 0.0 and np.all(np.diff(P.exp_ref(w)) <= 0)


def test_draw_tape_argument_checks_run_before_any_launch():
    """Host-side checks of gg_ccdm_draw_tape, callable without a GPU; the draw loop stands once in csrc/."""
    import os
    import re
    from util import load_lib
    lib = load_lib()
    one = 1                                                  # any non-NULL address: no check dereferences it
    assert lib.gg_ccdm_draw_tape(0, None, 0, None, 16, 8, None, None, None, None) != 0 and b"no output" in lib.gg_last_error()
    assert lib.gg_ccdm_draw_tape(0, None, 0, None, 24, 8, None, one, None, None) != 0 and b"kmax=24" in lib.gg_last_error()
    assert lib.gg_ccdm_draw_tape(0, one, 3, None, 16, 8, None, one, None, None) != 0 and b"not a multiple" in lib.gg_last_error()
    assert lib.gg_ccdm_draw_tape(0, one, 0, None, 32, 8, None, one, None, None) != 0
    assert lib.gg_ccdm_draw_tape(0, None, 0, None, 32, 0, None, one, None, None) == 0        # nothing to draw
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jointimagegeneration_amd", "csrc")
    calls = {f: len(re.findall(r"\bphilox4x32_10\s*\(", open(os.path.join(csrc, f)).read())) for f in sorted(os.listdir(csrc))
             if f.endswith((".hip", ".h", ".inc"))}
    assert {f: n for f, n in calls.items() if n} == {"gg_posterior.h": 2}, calls            # its definition and the call in ccdm_draw_row


@pytest.mark.parametrize("fault", P.FAULTS)
def test_compared_inputs_catch_each_emulated_fault(fault):
    """Each defect changes at least one word, and at least one label of an equal-probability race, of the launches the GPU test compares
    (the key swap cannot show at seed 0, whose two key words are equal, the row reduction only in per-sample mode, the offset only at an
    offset != 0: so the count of the cases that see it is asserted to be what that reasoning gives, not merely non-zero)."""
    seen_words = seen_labels = 0
    for kmax, kw in P.word_cases():
        good, bad = P.draw_words(kmax=kmax, **kw), P.draw_words(kmax=kmax, fault=fault, **kw)
        seen_words += int(not np.array_equal(good, bad))
        K = 14 if kmax == 16 else 32
        seen_labels += int(not np.array_equal(P.race_labels(good, K), P.race_labels(bad, K)))
    n = len(P.word_cases())
    per_sample = sum(1 for _, kw in P.word_cases() if "seeds" in kw)
    with_offset = sum(1 for _, kw in P.word_cases() if kw["offset"] is not None)
    with_key = sum(1 for _, kw in P.word_cases() if kw.get("seed", 1) != 0)              # seed 0: both key words equal
    expect = {"wrong_multiplier": n, "key_words_swapped": with_key, "counter_words_2_3_swapped": n, "q4_from_1": n,
              "row_not_reduced": per_sample, "offset_ignored": with_offset}[fault]
    assert seen_words == expect and seen_labels == expect, (fault, seen_words, seen_labels, expect)
    assert expect >= 6
