"""CIDEr-D (Vedantam et al. 2015) over token-id sequences: the sentence reward of self-critical sequence training.

For n = 1..4 a sentence is the vector of its n-gram counts weighted by ``log(N) - log(max(1, df))``, ``df`` the number
of training images whose references contain the n-gram and ``N`` the number of images.  A hypothesis is compared
with each reference of its image by a cosine in which the hypothesis' weight is clipped at the reference's, times a
Gaussian penalty ``exp(-(len_h - len_r)^2 / (2 sigma^2))`` (sigma = 6) on the length difference; the score is the
mean over n and over the references, times 10.  It works on ids -- no tokenizer -- with start, pad and end tokens
stripped as ``bleu.decode_plain`` / ``decode_bert`` delimit a sentence: start and pad ids are dropped and the sentence
ends before the first end id.  Pure Python on the host.
"""
import math
from collections import Counter

PLAIN_IDS = dict(start_id=0, end_id=1, pad_id=3)          # generate_json_data.py:45-48
BERT_IDS = dict(start_id=101, end_id=102, pad_id=0)


def strip_ids(seq, start_id, end_id, pad_id):
    """The sentence's words: start and pad ids dropped, cut before the first end id."""
    out = []
    for t in seq:
        t = int(t)
        if t == end_id:
            break
        if t != start_id and t != pad_id:
            out.append(t)
    return out


def _ngrams(words, n_max):
    c = Counter()
    for n in range(1, n_max + 1):
        for i in range(len(words) - n + 1):
            c[tuple(words[i:i + n])] += 1
    return c


class CiderD:
    """``CiderD(all_captions, start_id, end_id, pad_id)``: ``all_captions[i]`` holds the reference sentences (id
    sequences) of training image ``i``; document frequencies are counted once, here.  ``score(hypotheses,
    image_indices)`` returns one float per hypothesis, scored against the references of its image."""

    N_MAX, SIGMA, FACTOR = 4, 6.0, 10.0

    def __init__(self, all_captions, start_id=0, end_id=1, pad_id=3):
        self.ids = (int(start_id), int(end_id), int(pad_id))
        self.refs = [[strip_ids(r, *self.ids) for r in refs] for refs in all_captions]
        self.ref_counts = [[_ngrams(r, self.N_MAX) for r in refs] for refs in self.refs]
        self.df = Counter()
        for counts in self.ref_counts:
            for ng in set().union(*counts) if counts else ():
                self.df[ng] += 1
        self.log_n = math.log(max(1, len(self.refs)))
        self._ref_vecs = {}

    def _vec(self, counts):
        """per n: {n-gram: tf-idf weight}, and the vector's norm"""
        vec = [dict() for _ in range(self.N_MAX)]
        norm = [0.0] * self.N_MAX
        for ng, tf in counts.items():
            w = tf * (self.log_n - math.log(max(1, self.df.get(ng, 0))))
            vec[len(ng) - 1][ng] = w
            norm[len(ng) - 1] += w * w
        return vec, [math.sqrt(x) for x in norm]

    def _refs_of(self, i):
        if i not in self._ref_vecs:
            self._ref_vecs[i] = [self._vec(c) + (len(r),) for c, r in zip(self.ref_counts[i], self.refs[i])]
        return self._ref_vecs[i]

    def score_one(self, hypothesis, image_index):
        words = strip_ids(hypothesis, *self.ids)
        refs = self._refs_of(int(image_index))
        if not words or not refs:
            return 0.0
        vec_h, norm_h = self._vec(_ngrams(words, self.N_MAX))
        total = 0.0
        for vec_r, norm_r, len_r in refs:
            penalty = math.exp(-((len(words) - len_r) ** 2) / (2.0 * self.SIGMA ** 2))
            for n in range(self.N_MAX):
                if norm_h[n] == 0.0 or norm_r[n] == 0.0:
                    continue
                dot = sum(min(w, vec_r[n][ng]) * vec_r[n][ng] for ng, w in vec_h[n].items() if ng in vec_r[n])
                total += dot / (norm_h[n] * norm_r[n]) * penalty
        return self.FACTOR * total / (self.N_MAX * len(refs))

    def score(self, hypotheses, image_indices):
        return [self.score_one(h, i) for h, i in zip(hypotheses, image_indices)]
