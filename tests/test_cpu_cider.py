"""sat_amd.CiderD against a plainly written float64 restatement of CIDEr-D on a hand-built corpus: 6 images, 3
references each, a vocabulary of 12 words (ids 4..15; 0 = start, 1 = end, 3 = pad)."""
import math

import numpy as np
import pytest

import sat_amd

S, E, P = 0, 1, 3
EVERY = 4   # a word in some reference of every image: its idf is log(6) - log(6) = 0
CORPUS = [
    [[S, EVERY, 5, 6, 7, E, P, P], [S, 5, 6, 7, 8, E, P, P], [S, EVERY, 5, 9, E, P, P, P]],
    [[S, 6, 7, 8, 9, 10, E, P], [S, EVERY, 6, 7, E, P, P, P], [S, 10, 11, 12, E, P, P, P]],
    [[S, 12, 13, EVERY, E, P, P, P], [S, 12, 13, 14, 15, E, P, P], [S, 5, 13, 14, E, P, P, P]],
    [[S, EVERY, 14, 15, E, P, P, P], [S, 15, 14, 13, 12, 11, E, P], [S, 11, 10, 9, E, P, P, P]],
    [[S, 8, 8, 9, EVERY, E, P, P], [S, 8, 9, 10, 11, 12, 13, E], [S, 9, 8, 7, E, P, P, P]],
    [[S, 7, EVERY, 15, E, P, P, P], [S, 7, 15, 5, 6, E, P, P], [S, 15, 7, 10, 14, E, P, P]],
]


def _words(seq):
    out = []
    for t in seq:
        if t == E:
            break
        if t not in (S, P):
            out.append(t)
    return out


def _counts(words, n):
    c = {}
    for i in range(len(words) - n + 1):
        g = tuple(words[i:i + n])
        c[g] = c.get(g, 0) + 1
    return c


def restated_cider_d(corpus, hyp, image, sigma=6.0):
    """CIDEr-D, one n at a time, in float64 numpy vectors over the union of n-grams."""
    refs_all = [[_words(r) for r in refs] for refs in corpus]
    h = _words(hyp)
    if not h:
        return 0.0
    score = 0.0
    for n in range(1, 5):
        df = {}
        for refs in refs_all:
            seen = set()
            for r in refs:
                seen |= set(_counts(r, n))
            for g in seen:
                df[g] = df.get(g, 0) + 1
        idf = lambda g: math.log(len(corpus)) - math.log(max(1, df.get(g, 0)))  # noqa: E731
        ch = _counts(h, n)
        for r in refs_all[image]:
            cr = _counts(r, n)
            keys = sorted(set(ch) | set(cr))
            vh = np.array([ch.get(g, 0) * idf(g) for g in keys], dtype=np.float64)
            vr = np.array([cr.get(g, 0) * idf(g) for g in keys], dtype=np.float64)
            nh, nr = np.linalg.norm(vh), np.linalg.norm(vr)
            if nh == 0 or nr == 0:
                continue
            sim = float((np.minimum(vh, vr) * vr).sum() / (nh * nr))
            score += sim * math.exp(-((len(h) - len(r)) ** 2) / (2 * sigma ** 2))
    return 10.0 * score / (4 * len(refs_all[image]))


@pytest.fixture(scope="module")
def cider():
    return sat_amd.CiderD(CORPUS, start_id=S, end_id=E, pad_id=P)


def test_matches_the_restatement(cider):
    rng = np.random.default_rng(5)
    hyps, imgs = [], []
    for i, refs in enumerate(CORPUS):
        for r in refs:
            hyps.append(list(r)); imgs.append(i)                         # the references themselves
            hyps.append(list(r)); imgs.append((i + 1) % len(CORPUS))     # against another image
        for _ in range(4):                                               # random sentences
            n = int(rng.integers(1, 7))
            hyps.append([S] + [int(t) for t in rng.integers(4, 16, n)] + [E] + [P] * (6 - n)); imgs.append(i)
    got = cider.score(hyps, imgs)
    assert len(got) == len(hyps) and all(isinstance(x, float) for x in got)
    for h, i, g in zip(hyps, imgs, got):
        want = restated_cider_d(CORPUS, h, i)
        assert abs(g - want) <= 1e-12 * max(1.0, abs(want)), (h, i, g, want)
    assert max(got) > 1.0 and min(got) >= 0.0


def test_a_reference_beats_every_edit_of_it(cider):
    ref = CORPUS[2][1]                       # 12 13 14 15
    base = cider.score([ref], [2])[0]
    w = _words(ref)
    edits = [w[:-1], w[1:], w + [5], [w[1], w[0]] + w[2:], w[:1] + [9] + w[2:], w[:2] + [6] + w[2:]]
    for e in edits:
        s = cider.score([[S] + e + [E]], [2])[0]
        assert s < base, (e, s, base)


def test_a_repeated_ngram_is_clipped(cider):
    """The hypothesis' weight is clipped at the reference's: repeating a matching word adds nothing to the numerator
    and grows the norm."""
    once = cider.score([[S, 12, 13, E]], [2])[0]
    many = cider.score([[S, 12, 12, 12, 12, 13, E]], [2])[0]
    assert 0 < many < once
    # the unigram term alone, by hand, against reference [12, 13, 14, 15] of image 2: min(4 w, w) = w
    for hyp, img in (([S, 12, 12, 12, 12, 13, E], 2), ([S, 8, 8, 8, E], 4)):
        assert abs(cider.score([hyp], [img])[0] - restated_cider_d(CORPUS, hyp, img)) < 1e-12


def test_a_term_in_every_document_contributes_nothing(cider):
    assert all(any(EVERY in r for r in refs) for refs in CORPUS)
    assert cider.score([[S, EVERY, E]], [0])[0] == 0.0
    # adding it changes a score only through the length penalty and the higher-order n-grams it breaks: appended at
    # the end of a one-word sentence it adds a zero-weight unigram and one unseen bigram
    a = cider.score([[S, 5, E]], [0])[0]
    b = cider.score([[S, 5, EVERY, E]], [0])[0]
    want = restated_cider_d(CORPUS, [S, 5, EVERY, E], 0)
    assert abs(b - want) < 1e-12 and a > 0
    # the unigram part of b is a's cosine under the penalty of a two-word sentence
    uni_a = restated_cider_d(CORPUS, [S, 5, E], 0)
    assert abs(a - uni_a) < 1e-12


def test_length_penalty_follows_the_gaussian():
    """One reference, hypotheses that repeat its single informative word: the cosine is 1 for the unigrams, so the score
    is the Gaussian of the length difference."""
    corpus = [[[S, 5, E]], [[S, 6, E]], [[S, 7, E]]]
    c = sat_amd.CiderD(corpus, start_id=S, end_id=E, pad_id=P)
    base = c.score([[S, 5, E]], [0])[0]
    assert abs(base - 10.0 / 4) < 1e-12           # unigrams match exactly; no 2..4-grams in a one-word sentence
    for extra in (1, 2, 5):
        # [5, 5, ...]: unigram vector parallel to the reference's, clipped to it: cosine = w * w / (k w * w) = 1 / k
        k = 1 + extra
        s = c.score([[S] + [5] * k + [E]], [0])[0]
        assert abs(s - 10.0 / 4 / k * math.exp(-(extra ** 2) / 72.0)) < 1e-12, (extra, s)


def test_empty_hypothesis_scores_zero(cider):
    assert cider.score([[S, E, P, P], [E], [], [P, P], [S]], [0, 1, 2, 3, 4]) == [0.0] * 5


def test_reference_order_does_not_matter(cider):
    rng = np.random.default_rng(9)
    shuffled = [[refs[j] for j in rng.permutation(len(refs))] for refs in CORPUS]
    other = sat_amd.CiderD(shuffled, start_id=S, end_id=E, pad_id=P)
    hyps = [CORPUS[i][0] for i in range(6)] + [[S, 7, 8, 9, 10, E], [S, 15, 14, E]]
    imgs = list(range(6)) + [1, 3]
    a, b = cider.score(hyps, imgs), other.score(hyps, imgs)
    assert all(abs(x - y) <= 1e-12 for x, y in zip(a, b))


def test_bert_ids_are_stripped_as_decode_bert_delimits_them():
    refs = [[[101, 2054, 2003, 0, 0, 102]], [[101, 2023, 2003, 0, 0, 102]], [[101, 2054, 2023, 2003, 0, 102]]]
    c = sat_amd.CiderD(refs, start_id=101, end_id=102, pad_id=0)
    assert c.refs[0] == [[2054, 2003]] and c.refs[2] == [[2054, 2023, 2003]]
    assert c.score([[101, 2054, 2003, 102, 0, 0]], [0])[0] == c.score([[2054, 2003]], [0])[0] > 0
