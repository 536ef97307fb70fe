"""Cases for the device CIDEr-D scorer (sat_amd.CiderDDevice, sat_cider_*): a corpus, hypothesis rows and image indices
each, small enough that scoring all of them on the GPU takes seconds.  No GPU is needed to build them; the yardstick
is the host sat_amd.CiderD (fp64), which tests/test_cpu_cider.py pins against an independent restatement.

A case is a ``Case``: ``corpus[i]`` the reference rows of image i, ``ids`` = (start, end, pad), ``tokens`` int32
[n, T1] the hypothesis rows, ``images`` int64 [n].  ``FAMILIES`` groups them; within every family the host scores span
exact zeros and non-zero values.
"""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name family corpus ids tokens images")

PLAIN = (0, 1, 3)
BERT = (101, 102, 0)
ID_LIMIT = 1 << 20


def _rows(hyps, T1, pad):
    out = np.full((len(hyps), T1), pad, dtype=np.int32)
    for i, h in enumerate(hyps):
        assert len(h) <= T1, (len(h), T1)
        out[i, :len(h)] = h
    return out


def _case(name, family, corpus, ids, hyps, images, T1):
    assert len(hyps) == len(images)
    return Case(name, family, corpus, ids, _rows(hyps, T1, ids[2]), np.asarray(images, dtype=np.int64))


# ---------------------------------------------------------------- 1. the hand-built corpus of tests/test_cpu_cider.py
S, E, P = PLAIN
EVERY = 4   # a word in some reference of every image: idf log 6 - log 6 = 0
HAND_CORPUS = [
    [[S, EVERY, 5, 6, 7, E, P, P], [S, 5, 6, 7, 8, E, P, P], [S, EVERY, 5, 9, E, P, P, P]],
    [[S, 6, 7, 8, 9, 10, E, P], [S, EVERY, 6, 7, E, P, P, P], [S, 10, 11, 12, E, P, P, P]],
    [[S, 12, 13, EVERY, E, P, P, P], [S, 12, 13, 14, 15, E, P, P], [S, 5, 13, 14, E, P, P, P]],
    [[S, EVERY, 14, 15, E, P, P, P], [S, 15, 14, 13, 12, 11, E, P], [S, 11, 10, 9, E, P, P, P]],
    [[S, 8, 8, 9, EVERY, E, P, P], [S, 8, 9, 10, 11, 12, 13, E], [S, 9, 8, 7, E, P, P, P]],
    [[S, 7, EVERY, 15, E, P, P, P], [S, 7, 15, 5, 6, E, P, P], [S, 15, 7, 10, 14, E, P, P]],
]


def hand_case():
    rng = np.random.default_rng(5)
    hyps, imgs = [], []
    for i, refs in enumerate(HAND_CORPUS):   # test_matches_the_restatement's set
        for r in refs:
            hyps.append(list(r)); imgs.append(i)
            hyps.append(list(r)); imgs.append((i + 1) % len(HAND_CORPUS))
        for _ in range(4):
            n = int(rng.integers(1, 7))
            hyps.append([S] + [int(t) for t in rng.integers(4, 16, n)] + [E] + [P] * (6 - n)); imgs.append(i)
    # ... and the sentences of that file's other tests: edits of a reference, clipped repeats, the zero-idf word, empties
    w = [12, 13, 14, 15]
    for e in (w[:-1], w[1:], w + [5], [w[1], w[0]] + w[2:], w[:1] + [9] + w[2:], w[:2] + [6] + w[2:]):
        hyps.append([S] + e + [E]); imgs.append(2)
    for h, i in (([S, 12, 13, E], 2), ([S, 12, 12, 12, 12, 13, E], 2), ([S, 8, 8, 8, E], 4), ([S, EVERY, E], 0),
                 ([S, 5, E], 0), ([S, 5, EVERY, E], 0), ([S, E, P, P], 0), ([E], 1), ([], 2), ([P, P], 3), ([S], 4)):
        hyps.append(h); imgs.append(i)
    return _case("hand", "hand", HAND_CORPUS, PLAIN, hyps, imgs, 8)


# ---------------------------------------------------------------- 2. random corpora
RANDOM = dict(images=200, hyps=256, max_refs=7, min_len=3, max_len=20, T1=24)


def random_case(V, seed):
    """200 images with 1..7 references of 3..20 words over V words (ids 4 .. V + 3); 256 hypotheses: a reference of the
    image, a single-word edit of one, a random sentence, in turn."""
    d = RANDOM
    rng = np.random.default_rng(seed)

    def sentence(n):
        return [int(t) for t in rng.integers(4, V + 4, n)]

    def row(words):
        return [S] + words + [E]

    counts = [1 + (i % d["max_refs"]) for i in range(d["images"])]   # every count from 1 to 7 occurs
    rng.shuffle(counts)
    corpus = [[row(sentence(int(rng.integers(d["min_len"], d["max_len"] + 1)))) for _ in range(k)] for k in counts]
    hyps, imgs = [], []
    for i in range(d["hyps"]):
        img = int(rng.integers(0, d["images"]))
        ref = corpus[img][int(rng.integers(0, len(corpus[img])))][1:-1]
        if i % 3 == 0:
            words = list(ref)
        elif i % 3 == 1:
            words = list(ref)
            words[int(rng.integers(0, len(words)))] = int(rng.integers(4, V + 4))
        else:
            words = sentence(int(rng.integers(1, d["max_len"] + 1)))
        hyps.append(row(words)); imgs.append(img)
    return _case(f"random_v{V}", "random", corpus, PLAIN, hyps, imgs, d["T1"])


# ---------------------------------------------------------------- 3. lengths, at T1 = 64
def lengths_case():
    rng = np.random.default_rng(11)
    w = lambda n: [int(t) for t in rng.integers(4, 40, n)]  # noqa: E731
    long64, long63 = w(64), w(63)
    corpus = [
        [[S, 10, 11, 12, 13, 14, E], [S, 10, 11, 12, 13, 14, 15, 16, 17, 18, E]],       # 5 and 9 words
        [long64, [S] + long63],                                                        # 64 and 63 words, no end id
        [[S, 20, 21, 22, E], [S, 22, 21, 20, E]],                                       # 3 words
        [[S, 30, 31, 32, 33, E], [S, 5, 6, E]],
        [[S] + w(12) + [E] for _ in range(3)],
    ]
    hyps = [
        ([], 0), ([S, E], 0), ([P] * 64, 0),                          # 0 words
        ([S, 10, E], 0), ([S, 39, E], 0),                             # 1 word: in a reference, in none
        ([S, 10, 11, 12, E], 0), ([S, 20, 21, 22, E], 2),             # 3 words: no 4-gram
        (long63 + [E], 1), ([S] + long63, 1),                         # 63 words
        (long64, 1), (long64[::-1], 1), (w(64), 4),                   # 64 words: the row is all words
        ([E, 10, 11, 12, 13, 14], 0), ([E] + long63, 1),              # the end id at position 0
        ([S, 10, 11, 12, 13, 14], 0), ([S, 30, 31, 32, 33] + [P] * 20, 3), (long63, 1),      # no end id at all
        ([S, 10, 11, P, 12, S, 13, P, P, 14, E], 0), ([P, S, 30, P, 31, 32, S, 33, E, 5, 6], 3),   # start / pad inside
        ([S, 10, P, 12, E], 0),                                       # (10, 12) is a bigram of no reference
        ([S] + [20, 21, 22] * 20 + [E], 2), ([S] + w(60) + [E], 2), ([S] + [5, 6] * 30, 3),  # far longer than the refs
    ]
    return _case("lengths", "lengths", corpus, PLAIN, [h for h, _ in hyps], [i for _, i in hyps], 64)


# ---------------------------------------------------------------- 4. ids
def bert_case():
    s, e, p = BERT
    corpus = [
        [[s, 2054, 2003, 1996, 3899, e, p, p], [s, 1037, 3899, 2003, 2770, e, p, p]],
        [[s, 2023, 2003, 1037, 4937, e, p, p], [s, 1996, 4937, 2938, 2006, 1996, 13523, e]],
        [[s, 2054, 2023, 2003, e, p, p, p]],
        [[s, 30521, 1037, 30521, e, p, p, p], [s, 1037, 2158, 5559, 1037, 3586, e, p]],
    ]
    hyps = [([s, 2054, 2003, 1996, 3899, e], 0), ([s, 2054, 2003, 1996, 4937, e], 0), ([s, 1037, 3899, e, 2003], 0),
            ([s, 1996, 4937, 2938, e], 1), ([s, 2023, p, 2003, 1037, 4937, e], 1), ([s, 2054, 2023, 2003, e], 2),
            ([s, 2054, 2023, 2003, e], 0), ([s, 30521, 1037, 30521, e], 3), ([s, 30521, 30521, e], 3),
            ([s, 29999, 29998, e], 3), ([s, e], 1), ([p, p, p], 2), ([s, 1037, 2158, 5559, 1037, 3586, e], 3)]
    return _case("bert", "ids", corpus, BERT, [h for h, _ in hyps], [i for _, i in hyps], 8)


def high_ids_case():
    a, b = ID_LIMIT - 1, ID_LIMIT - 2
    corpus = [
        [[S, a, b, a, b, E], [S, b, b, a, 5, E]],
        [[S, a, a, a, a, E], [S, 5, 6, a, E]],
        [[S, b, 5, b, 6, E]],
        [[S, 6, 5, E], [S, 5, b, E]],
    ]
    hyps = [([S, a, b, a, b, E], 0), ([S, a, b, a, E], 0), ([S, b, a, b, a, E], 0), ([S, a, a, a, a, E], 1),
            ([S, a, a, b, a, E], 1), ([S, b, 5, b, 6, E], 2), ([S, b, 5, a, 6, E], 2), ([S, a, E], 3), ([S, 5, b, E], 3),
            ([S, a - (1 << 19), E], 3), ([S, 7, 8, E], 0), ([S, b, b, a, 5, E], 0)]
    return _case("high_ids", "ids", corpus, PLAIN, [h for h, _ in hyps], [i for _, i in hyps], 8)


ZERO_WORD_IDS = (1000, 1001, 1002)


def zero_word_case():
    """start / end / pad = 1000 / 1001 / 1002: id 0 is a word.  The references hold the unigram (7) and the bigram
    (7, 0); a table that did not store n would mistake one for the other."""
    s, e, p = ZERO_WORD_IDS
    corpus = [
        [[s, 7, e, p, p, p], [s, 9, 7, e, p, p]],            # (7) without a following 0
        [[s, 7, 0, e, p, p], [s, 7, 0, 0, 0, e]],            # (7, 0), (7, 0, 0), (7, 0, 0, 0), (0, 0), ...
        [[s, 0, 5, e, p, p]],                                # (0) elsewhere
        [[s, 5, 6, 8, e, p]],
    ]
    hyps = [([s, 7, e], 0), ([s, 7, 0, e], 0), ([s, 7, e], 1), ([s, 7, 0, e], 1), ([s, 7, 0, 0, e], 1),
            ([s, 7, 0, 0, 0, e], 1), ([s, 0, e], 1), ([s, 0, 0, 0, 0, e], 1), ([s, 0, 5, e], 2), ([s, 0, e], 3),
            ([s, 3, 1, e], 0), ([s, 5, 6, 8, e], 3), ([s, 9, 7, 0, e], 0)]
    return _case("zero_word", "ids", corpus, ZERO_WORD_IDS, [h for h, _ in hyps], [i for _, i in hyps], 6)


# ---------------------------------------------------------------- 5. degenerate
def one_image_case():
    """log N = 0: every weight, hence every score, is exactly 0."""
    corpus = [[[S, 5, 6, 7, E], [S, 6, 7, 8, E]]]
    hyps = [[S, 5, 6, 7, E], [S, 6, 7, E], [S, 9, E], [S, E], [S, 5, 5, 5, 5, 5, E]]
    return _case("one_image", "degenerate", corpus, PLAIN, hyps, [0] * len(hyps), 8)


def no_refs_case():
    """The hand corpus and a seventh image without references: exactly 0 there, the others scored with N = 7."""
    corpus = HAND_CORPUS + [[]]
    hyps = [([S, 5, 6, 7, E], 6), ([S, EVERY, E], 6), ([S, 5, 6, 7, E], 0), ([S, 12, 13, 14, 15, E], 2), ([], 6)]
    return _case("no_refs", "degenerate", corpus, PLAIN, [h for h, _ in hyps], [i for _, i in hyps], 8)


def every_image_word_case():
    hyps = [([S, EVERY, E], i) for i in range(6)] + [([S, EVERY, EVERY, EVERY, E], 0), ([S, 5, EVERY, E], 0)]
    return _case("every_image_word", "degenerate", HAND_CORPUS, PLAIN, [h for h, _ in hyps], [i for _, i in hyps], 8)


def gaussian_case():
    """test_length_penalty_follows_the_gaussian: one reference per image, hypotheses that repeat its single word."""
    corpus = [[[S, 5, E]], [[S, 6, E]], [[S, 7, E]]]
    hyps = [[S] + [5] * k + [E] for k in (1, 2, 3, 6)]
    return _case("gaussian", "degenerate", corpus, PLAIN, hyps, [0] * len(hyps), 8)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [hand_case(), random_case(50, 21), random_case(5000, 22), lengths_case(), bert_case(), high_ids_case(),
             zero_word_case(), one_image_case(), no_refs_case(), every_image_word_case(), gaussian_case()]
    return {c.name: c for c in cases}


FAMILIES = ("hand", "random", "lengths", "ids", "degenerate")
NAMES = ("hand", "random_v50", "random_v5000", "lengths", "bert", "high_ids", "zero_word", "one_image", "no_refs",
         "every_image_word", "gaussian")

_HOST = {}


def host(name):
    """(the case's host CiderD, its fp64 scores as a numpy vector), computed once and left unchanged."""
    if name not in _HOST:
        import sat_amd
        c = all_cases()[name]
        cider = sat_amd.CiderD(c.corpus, *c.ids)
        scores = np.array(cider.score(c.tokens.tolist(), c.images.tolist()), dtype=np.float64)
        scores.setflags(write=False)
        _HOST[name] = (cider, scores)
    return _HOST[name]


def gaussian_expected():
    return np.array([10.0 / 4 / k * np.exp(-((k - 1) ** 2) / 72.0) for k in (1, 2, 3, 6)])
