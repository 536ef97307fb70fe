"""The device CIDEr-D cases (tests/cider_cases.py) without a GPU: they are well-formed, the host scores of every family
span exact zeros and non-zero values (a kernel returning zeros, or never returning one, cannot pass the GPU tests), the
key packing is the header's, and the library exports the four sat_cider_* entries."""
import math

import numpy as np
import pytest

import cider_cases as C
import sat_amd
from sat_amd import cider_device as CD


def test_library_exports_the_cider_entries():
    lib = sat_amd._lib.lib()
    for name in ("sat_cider_table_insert", "sat_cider_lookup", "sat_cider_ref_norms", "sat_cider_score"):
        assert hasattr(lib, name), name
        assert name in sat_amd._lib.EXPORTED
    assert sat_amd.CiderDDevice is CD.CiderDDevice


def test_names_and_families():
    cases = C.all_cases()
    assert tuple(cases) == C.NAMES
    assert {c.family for c in cases.values()} == set(C.FAMILIES)


@pytest.mark.parametrize("name", C.NAMES)
def test_case_is_well_formed(name):
    c = C.all_cases()[name]
    n, T1 = c.tokens.shape
    assert c.tokens.dtype == np.int32 and c.images.dtype == np.int64 and c.images.shape == (n,)
    assert 1 <= T1 <= 64 and n >= 4
    assert c.images.min() >= 0 and c.images.max() < len(c.corpus)
    assert c.tokens.min() >= 0 and c.tokens.max() < C.ID_LIMIT
    cider, scores = C.host(name)
    assert scores.shape == (n,) and np.isfinite(scores).all() and (scores >= 0).all()
    assert max((len(r) for refs in cider.refs for r in refs), default=0) <= 64
    assert all(0 <= t < C.ID_LIMIT for refs in cider.refs for r in refs for t in r)
    assert len(set(c.ids)) == 3


@pytest.mark.parametrize("family", C.FAMILIES)
def test_family_spans_zero_and_nonzero(family):
    scores = np.concatenate([C.host(n)[1] for n, c in C.all_cases().items() if c.family == family])
    assert (scores == 0.0).any() and (scores > 0.1).any(), (family, scores.min(), scores.max())


def test_random_corpora_are_uneven_dense_and_sparse():
    for name, dense in (("random_v50", True), ("random_v5000", False)):
        c = C.all_cases()[name]
        assert len(c.corpus) == 200 and c.tokens.shape == (256, 24)
        counts = sorted({len(refs) for refs in c.corpus})
        assert counts == [1, 2, 3, 4, 5, 6, 7]
        cider, scores = C.host(name)
        hyp_words = [sat_amd.cider.strip_ids(h, *c.ids) for h in c.tokens.tolist()]
        absent = sum(1 for w in hyp_words for i in range(len(w) - 1) if tuple(w[i:i + 2]) not in cider.df)
        bigrams = sum(max(0, len(w) - 1) for w in hyp_words)
        repeats = sum(1 for w in hyp_words if len(set(w)) < len(w))
        ref_repeats = sum(1 for refs in cider.refs for r in refs if len(set(r)) < len(r))
        if dense:   # tf > 1 on both sides
            assert repeats > 50 and ref_repeats > 100
        else:       # many hypothesis n-grams the table does not hold
            assert absent > bigrams // 4
        assert (scores == 0).sum() >= (0 if dense else 20) and (scores > 1).sum() > 80


def test_lengths_case_covers_the_stated_lengths():
    c = C.all_cases()["lengths"]
    lens = [len(sat_amd.cider.strip_ids(h, *c.ids)) for h in c.tokens.tolist()]
    assert {0, 1, 3, 63, 64} <= set(lens) and c.tokens.shape[1] == 64
    s, e, p = c.ids
    rows = c.tokens.tolist()
    assert any(r[0] == e for r in rows) and any(e not in r for r in rows)
    inside = [r for r in rows if e in r and any(t in (s, p) for t in r[1:r.index(e)]) and r.index(e) > 2]
    assert inside
    longest_ref = {i: max(len(r) for r in refs) for i, refs in enumerate(C.host("lengths")[0].refs)}
    assert any(n >= 10 * longest_ref[int(i)] for n, i in zip(lens, c.images))
    assert max(longest_ref.values()) == 64
    # an n-gram spans a dropped token: dropping the pad inside (10, P, 12) makes the bigram (10, 12)
    cider, scores = C.host("lengths")
    row = rows.index([s, 10, p, 12, e] + [p] * 59)
    assert scores[row] == cider.score([[10, 12]], [0])[0] > 0


def test_zero_word_case_tells_the_unigram_from_the_bigram():
    cider, scores = C.host("zero_word")
    assert (7,) in cider.df and (7, 0) in cider.df and (0,) in cider.df and (7, 0, 0, 0) in cider.df
    assert cider.df[(7,)] != cider.df[(7, 0)]
    c = C.all_cases()["zero_word"]
    by = {(tuple(sat_amd.cider.strip_ids(h, *c.ids)), int(i)): s for h, i, s in zip(c.tokens.tolist(), c.images, scores)}
    assert by[((7,), 0)] != by[((7, 0), 0)] and by[((7,), 1)] != by[((7, 0), 1)]
    assert by[((7, 0), 1)] > by[((7,), 1)] > 0


def test_degenerate_cases_score_what_they_say():
    assert (C.host("one_image")[1] == 0.0).all() and C.host("one_image")[0].log_n == 0.0
    nr = C.host("no_refs")[1]
    assert (nr[[0, 1, 4]] == 0.0).all() and (nr[[2, 3]] > 0).all()
    ev = C.host("every_image_word")[1]
    assert (ev[:7] == 0.0).all() and ev[7] > 0
    assert np.abs(C.host("gaussian")[1] - C.gaussian_expected()).max() < 1e-12


def test_key_packing_is_the_headers():
    k = CD.pack_keys([(7,), (7, 0), (1, 2, 3, 4), (C.ID_LIMIT - 1,) * 4, (0, 0, 0x12345)])
    assert k.dtype == np.uint32 and k.shape == (5, 3)
    assert k[0].tolist() == [1 << 20 | 7, 0, 0] and k[1].tolist() == [2 << 20 | 7, 0, 0]
    assert k[2].tolist() == [4 << 20 | 1, 2 | 3 << 20, 4 << 8]
    assert k[3].tolist() == [4 << 20 | 0xfffff, 0xffffffff, 0x0fffffff]
    assert k[4].tolist() == [3 << 20, 0x345 << 20, 0x12]
    assert len({tuple(r) for r in k.tolist()}) == 5 and (k[:, 0] != 0).all()
    for bad in ([()], [(1, 2, 3, 4, 5)], [(C.ID_LIMIT,)], [(-1,)]):
        with pytest.raises(ValueError):
            CD.pack_keys(bad)
    assert CD.default_table_slots(0) == 16 and CD.default_table_slots(8) == 16 and CD.default_table_slots(9) == 32
    assert CD.default_table_slots(100000) == 262144 and math.log2(CD.default_table_slots(12345)).is_integer()
