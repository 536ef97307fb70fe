"""The batched beam-search fixtures (beam_batch_fixtures.py) are fit for an ids comparison: the
oracle's fp32 and fp64 searches pick the same words for every image (no top-k margin inside
rounding noise), set A holds the cases the device tests need, and the golden image's oracle result
is the stored reference sentence.  No GPU."""
import math

import pytest

import beam_batch_fixtures as FX


@pytest.mark.parametrize("max_step", FX.MAX_STEPS)
@pytest.mark.parametrize("name", sorted(FX.SETS))
def test_fp32_and_fp64_oracle_agree(name, max_step):
    """A seed that disagrees is a fixture whose margins are inside rounding noise: replace it."""
    e32, e64 = FX.expected(name, max_step), FX.expected(name, max_step, True)
    g, feats = FX.load(name)
    assert len(e32) == len(e64) == feats.shape[0] == 1 + len(FX.SETS[name][1])
    for i, (a, b) in enumerate(zip(e32, e64)):
        assert a[0] == b[0], (name, i)
        assert a[1].shape == b[1].shape
        assert math.isinf(a[2]) == math.isinf(b[2])


def test_set_sizes():
    sizes = {n: (FX.load(n)[1].shape[0], FX.load(n)[0]["cfg"]["beam"]) for n in FX.SETS}
    assert sizes == {"A": (7, 3), "B_ado": (4, 5), "B_noatt": (3, 4), "B_bert": (5, 3), "beam1": (1, 1)}


def test_set_a_covers_the_cases():
    short = FX.expected("A", 6)
    assert any(math.isinf(s) for _, _, s in short) and any(not math.isinf(s) for _, _, s in short)
    for ids, al, s in short:
        if math.isinf(s):   # no completed sentence: [0] and the last step's beam-many alpha rows
            assert ids == [0] and al.shape[0] == 3
        else:
            assert 2 <= len(ids) <= 8 and al.shape[0] == len(ids)
    assert any(len(ids) == 8 for ids, _, _ in short)   # a beam that completes at the last step allowed
    full = FX.expected("A", 50)
    assert len({len(ids) for ids, _, s in full if not math.isinf(s)}) >= 3
    assert any(math.isinf(s) for _, _, s in full)      # and one image that never completes in 51 steps


@pytest.mark.parametrize("name", sorted(FX.SETS))
def test_golden_image_matches_stored_sentence(name):
    g, _ = FX.load(name)
    ids, al, score = FX.expected(name, 50)[0]
    assert ids == g["sentence"].tolist()
    assert al.shape == tuple(g["alphas"].shape)
