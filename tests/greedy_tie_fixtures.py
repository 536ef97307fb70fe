"""Fixtures that pin the greedy feedback argmax (decoder.py:132, ``output.max(1)[1]``) on planted exact ties, in every
kernel form.  test_cpu_greedy_tie_fixtures.py qualifies them with the oracle alone, test_gpu_greedy_ties.py runs them
on the device.

The rule is ``sat_argmax_better`` (csrc/sat_internal.h): value descending, then the lower index; NaN above everything,
the first NaN wins.  Five reductions apply it ("greedy feedback: the tie rule and where it is applied"):
``argmax_kernel`` (per-op; 16-byte vectors on aligned rows, scalar loads elsewhere), ``head_out_kernel`` and
``head_out_lds_kernel`` (the fused step's vocabulary heads: per-block partials), the token fold of the LSTM kernel over
those partials, and ``sampled_finish_kernel`` (the same fold, 64 threads, the sample form's last step).

Every logit here is a small integer (|x| <= 64): exact in fp32, in fp64, in bf16 and in any summation order, so tokens
AND logits are compared with ``==`` and every expected token follows by hand from the pattern's description.

A PATTERN is a vector of V integers: ``low`` everywhere and plateaus ``(value, words)`` on top.  Its kinds:

  pair(i, j)       words i < j share the top value, a lower plateau lies elsewhere: i must win, by the index rule alone
  top(w)           w alone on top, the lower plateau's tie earlier
  vbi(w, lows)     VALUE BEATS INDEX: w alone on top at a high index, a tie one value lower at the earlier ``lows``
  allneg           every value negative: the ado head's ReLU makes every logit 0 and token 0 wins

Ado head: a CHAIN of patterns in one forward.  f_h, f_z (weights and biases) and f_out.bias are zero, so the head's
``combined`` is exactly the fed token's embedding row; embedding.weight[w] is one-hot at ``pat(w)`` and
f_out.weight[:, k] holds pattern k (the other columns zero), so ``preds[b, t] = relu(pattern pat(fed token))``.
``pat(start token) = 0`` and ``pat(winner of pattern k) = k + 1``: step t shows pattern t to every row, through the
real feedback.  Every other word w has ``pat(w) = w % n`` (n patterns).  A pattern whose winner is token 0 goes last.
A chain runs ``steps`` = T - 1 steps: n + 1 (the last step shows pattern 0 again, so the last pattern's winner is a fed
token) or n (the last pattern is reduced only where the last step is: the sample form; that is where the claims of
``sampled_finish_kernel`` sit).  The embedding also feeds the LSTM, so h and the alphas are ordinary numbers: not
asserted.

Simple head: deep_output.weight zero, deep_output.bias the pattern; no embedding term, every step shows the same
pattern.  No ReLU: the place of the non-finite patterns (NaN at two words behind a +inf -> the first NaN; all -inf -> 0;
two +inf -> the lower).  The device's ReLU heads map a NaN pre-activation to 0 where torch keeps NaN: no NaN pattern
for the ado head.

Select form (scheduled sampling with the ``tf_mask`` hook): a row that keeps its caption token shows
``pat(caps[b, t])``, so the rows of one launch show different patterns (``select_inputs``).

CLAIMS state, as data, which boundary of which reduction a pattern straddles; test_cpu_greedy_tie_fixtures.py
recomputes every one from V, the block sizes and the dtype (``locate``), and the per-op path of every step from
``((T-1) V esz) % 16`` and ``(t V esz) % 16`` (``perop_path``).

Vocabularies: 16500 (> 16384: the folds' second trip and the vector path's second pass; % 4 == 0, % 8 != 0, % 64 != 0:
fp32 rows always aligned, bf16 rows aligned at even steps of an even T - 1) and 1003 (odd: the scalar path, the heads'
scalar stores; at T - 1 = 8 the rows of steps 0 and 4 (fp32) and of step 0 (bf16) are aligned, which puts 1000..1002 in
the vector path's scalar tail).
"""
import functools

import numpy as np
import torch

from oracle import sat_oracle as O

D, L = 64, 16
WSEED, FSEED, MSEED = 401, 402, 403


# ---- patterns ---------------------------------------------------------------------------------------------------
def pair(i, j):
    return ("pair", i, j)


def top(w):
    return ("top", w)


def vbi(w, lows):
    return ("vbi", w, tuple(lows))


ALLNEG = ("allneg",)


def plateaus_of(spec, V):
    """(low, ((value, words), ...)) of a pattern spec, top plateau first."""
    kind = spec[0]
    if kind == "allneg":
        return -3, ((-1, (1, 7)),)
    if kind == "pair":
        tops = ((2, (spec[1], spec[2])),)
    elif kind == "top":
        tops = ((2, (spec[1],)),)
    elif kind == "vbi":
        tops = ((3, (spec[1],)), (2, spec[2]))
    else:
        raise ValueError(spec)
    used = {w for _, ws in tops for w in ws}
    under = tuple(w for w in (1, 2, V - 2) if w not in used)
    return -2, tops + ((1, under),)


def vector_of(spec, V):
    """The pattern as a float64 array [V]."""
    low, plateaus = plateaus_of(spec, V)
    x = np.full(V, float(low))
    for value, words in reversed(plateaus):
        x[list(words)] = float(value)
    return x


def winner(x, rule="lower"):
    """The argmax of a pattern vector.  rule "lower": the device's rule, restated (value descending, then the lower
    index; NaN above everything, first NaN).  The WRONG rules the planted patterns must expose: "higher" (value, then
    the HIGHER index: a ``>=`` for a ``>``, a loop that keeps the later candidate) and "first_ge" (the first word at or
    above the runner-up value: an index that beats a value)."""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    if rule == "first_ge":
        vals = np.unique(x[~nan])
        return int(np.flatnonzero(nan | (x >= vals[-2 if len(vals) > 1 else -1]))[0])
    idx = np.flatnonzero(nan) if nan.any() else np.flatnonzero(x == x.max())
    return int(idx[0] if rule == "lower" else idx[-1])


# ---- chains (ado head) ------------------------------------------------------------------------------------------
CHAINS = {
    # wrap chains: 7 patterns, 8 steps; the last winner is token 0 and step 7 shows pattern 0 again
    "v16500_a": dict(V=16500, steps=8, patterns=(pair(2047, 2048), pair(63, 64), pair(15, 16), pair(255, 256),
                                                 pair(511, 512), pair(70, 326), pair(0, 16499))),
    "v16500_b": dict(V=16500, steps=8, patterns=(pair(5, 2053), pair(3, 4), pair(6, 16390), pair(31, 32),
                                                 pair(100, 16497), pair(7, 1031), ALLNEG)),
    # 8 patterns, 8 steps: the last one is reduced by the sample form only
    "v16500_c": dict(V=16500, steps=8, patterns=(top(16499), pair(8191, 8192), vbi(16393, (9, 10)), pair(4095, 4096),
                                                 vbi(11, (8, 9)), pair(8, 8200), pair(16, 17), pair(12, 4108))),
    "v16500_d": dict(V=16500, steps=2, patterns=(pair(16383, 16384), pair(4095, 4096))),
    "v1003_a": dict(V=1003, steps=8, patterns=(pair(100, 1001), pair(63, 64), pair(255, 256), pair(70, 326),
                                               top(1002), vbi(582, (70, 326)), ALLNEG)),
    "v1003_b": dict(V=1003, steps=8, patterns=(top(1002), pair(3, 4), pair(15, 16), pair(31, 32), pair(999, 1000),
                                               pair(995, 1000), pair(0, 1002))),
}
CHAINS_OF = {16500: ("v16500_a", "v16500_b", "v16500_c", "v16500_d"), 1003: ("v1003_a", "v1003_b")}


@functools.lru_cache(maxsize=None)
def chain(name):
    """The chain with everything derived: ``vectors`` [n, V] float64, ``winners`` (one per pattern), ``pat`` [V] int64
    (the pattern a fed word shows), ``shown`` / ``tokens`` / ``win`` per step of a plain greedy forward."""
    c = dict(CHAINS[name])
    V, n, T1 = c["V"], len(c["patterns"]), c["steps"]
    assert T1 in (n, n + 1)
    vectors = np.stack([vector_of(s, V) for s in c["patterns"]])
    winners = [winner(np.maximum(v, 0.0)) for v in vectors]   # the head's ReLU
    pat = np.arange(V, dtype=np.int64) % n
    for k, w in enumerate(winners[:-1]):
        pat[w] = k + 1
    shown = [t if t < n else int(pat[winners[-1]]) for t in range(T1)]
    c.update(name=name, n=n, vectors=vectors, winners=winners, pat=pat, shown=shown,
             tokens=[0] + [winners[k] for k in shown[:-1]], win=[winners[k] for k in shown])
    return c


# ---- simple head ------------------------------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
# name: (low, plateaus); V - k words are written as negative indices
SIMPLE_PATTERNS = {
    "pair_63_64": (-4, ((2, (63, 64)), (1, (1, 2)))),               # negative logits below the plateaus: no ReLU here
    "last_alone": (-2, ((-1, (-1,)),)),                              # V - 1 alone on top, every value negative
    "nan_behind_inf": (0, ((NAN, (200, -3)), (INF, (10,)), (1, (5,)))),   # -> 200, the first NaN
    "all_minus_inf": (-INF, ()),                                     # -> 0
    "two_inf": (0, ((INF, (70, -1)), (2, (3,)))),                    # -> 70
}
SIMPLE_V = (16500, 1003)
SIMPLE_STEPS = {16500: 4, 1003: 5}   # bf16 per-op at 16500: steps 0, 2 vector, step 1 scalar; 1003: never aligned


def simple_vector(name, V):
    low, plateaus = SIMPLE_PATTERNS[name]
    x = np.full(V, float(low))
    for value, words in reversed(plateaus):
        x[[w % V for w in words]] = value
    return x


# ---- parameters and inputs ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _base_params(V, E, ado):
    return O.make_decoder_params(V, D, E, ado, WSEED)


def chain_params(name, E):
    """fp32 state dict of a chain's decoder (ado head)."""
    c = chain(name)
    V, n = c["V"], c["n"]
    p = dict(_base_params(V, E, True))
    for k in ("f_h.weight", "f_h.bias", "f_z.weight", "f_z.bias", "f_out.bias"):
        p[k] = torch.zeros_like(p[k])
    emb = torch.zeros(V, E)
    emb[torch.arange(V), torch.from_numpy(c["pat"])] = 1.0
    w = torch.zeros(V, E)
    w[:, :n] = torch.from_numpy(c["vectors"].T.copy()).float()
    p["embedding.weight"], p["f_out.weight"] = emb, w
    return p


def simple_params(name, V, E):
    p = dict(_base_params(V, E, False))
    p["deep_output.weight"] = torch.zeros_like(p["deep_output.weight"])
    p["deep_output.bias"] = torch.from_numpy(simple_vector(name, V)).float()
    return p


def features(B):
    """[B, L, D] fp32, bf16-representable, every row its own: the logits must not depend on them."""
    x = np.maximum(np.random.default_rng(FSEED + B).standard_normal((B, L, D)), 0).astype(np.float32)
    return torch.from_numpy(x).bfloat16().float()


def dropout_masks(B, T1, E):
    """[T1, B, E] float keep masks as the oracle takes them (the device takes [B, T1, E] uint8)."""
    return O.make_dropout_masks(B, T1, E, MSEED + B)


def plain_captions(B, T1):
    """Captions of a greedy forward: only their length matters."""
    caps = torch.ones(B, T1 + 1, dtype=torch.long)
    caps[:, 0] = 0
    return caps


def select_inputs(name, B):
    """(caps [B, T] int64, keep [B, T-1] uint8) of the select form: row b keeps its caption token at step t >= 1 where
    (b + t) is even, and that token is the smallest non-winner word >= 40 showing pattern (b + 3 t) % n (so at an
    even step rows 0 and 2 keep two different patterns and row 1, kept one step earlier, shows a third)."""
    c = chain(name)
    n, T1, wins = c["n"], c["steps"], set(c["winners"])
    word = {q: next(w for w in range(40, c["V"]) if w % n == q and w not in wins) for q in range(n)}
    caps = plain_captions(B, T1)
    keep = torch.zeros(B, T1, dtype=torch.uint8)
    keep[:, 0] = 1
    for b in range(B):
        for t in range(1, T1):
            caps[b, t] = word[(b + 3 * t) % n]
            keep[b, t] = int((b + t) % 2 == 0)
    return caps, keep


def expected(name, B, select=False):
    """The hand-derived run of a chain: ``tokens`` [B, T1] (the fed tokens), ``shown`` [B, T1] (the pattern every row
    shows), ``win`` [B, T1] (its winner: what the sample form draws at temperature 0).  select: the host restatement
    -- the caption token where the mask keeps it, the previous winner elsewhere."""
    c = chain(name)
    T1, pat, winners = c["steps"], c["pat"], c["winners"]
    tokens = torch.zeros(B, T1, dtype=torch.long)
    if select:
        caps, keep = select_inputs(name, B)
        for t in range(1, T1):
            prev = torch.tensor([winners[pat[w]] for w in tokens[:, t - 1].tolist()])
            tokens[:, t] = torch.where(keep[:, t].bool(), caps[:, t], prev)
    else:
        tokens[:] = torch.tensor(c["tokens"])
    shown = torch.from_numpy(pat)[tokens]
    win = torch.tensor(winners)[shown]
    return dict(tokens=tokens, shown=shown, win=win)


def expected_preds(name, shown):
    """[B, T1, V] fp32: relu(pattern shown)."""
    return torch.from_numpy(np.maximum(chain(name)["vectors"], 0.0)).float()[shown]


# ---- where a word falls in a reduction ----------------------------------------------------------------------------
AM_THREADS, AM_NV = 256, 8             # argmax_kernel: threads, 16-byte vectors per thread and pass
SK_COLS, HO_BLK = 32, 64               # columns per partial: head_out_kernel, head_out_lds_kernel
FOLD_THREADS, FINISH_THREADS = 256, 64


def perop_path(V, T1, t, esz):
    """argmax_kernel's path for step t of a [B, T1, V] preds tensor (sat_argmax_rows: base and row stride aligned)."""
    return "vector" if (T1 * V * esz) % 16 == 0 and (t * V * esz) % 16 == 0 else "scalar"


def perop_paths(name, esz):
    """The path of every step of a chain's per-op forward: esz 4 (fp32) / 2 (bf16)."""
    c = chain(name)
    return [perop_path(c["V"], c["steps"], t, esz) for t in range(c["steps"])]


def head_blocks(V, E):
    """am_ncb: the partials per row (sat_greedy_head_blocks)."""
    blk = HO_BLK if E == 512 else SK_COLS
    return -(-V // blk)


def locate(red, w, V):
    """Where word w is reduced.  red: "vec4" / "vec8" (argmax_kernel's vector path, fp32 / bf16), "scalar", "head"
    (head_out_kernel), "lds" (head_out_lds_kernel), "fold32" / "fold64" (the LSTM kernel's fold over 32- / 64-column
    partials), "finish32" / "finish64" (sampled_finish_kernel)."""
    if red in ("vec4", "vec8"):
        vec = int(red[3:])
        nvec = V // vec
        if w >= nvec * vec:
            return dict(tail=True, thread=(w - nvec * vec) % AM_THREADS)
        vi = w // vec
        r = vi % (AM_THREADS * AM_NV)
        return dict(tail=False, vector=vi, trip=vi // (AM_THREADS * AM_NV), load=r // AM_THREADS,
                    thread=r % AM_THREADS, wave=r % AM_THREADS // 64)
    if red == "scalar":
        return dict(thread=w % AM_THREADS, trip=w // AM_THREADS, wave=w % AM_THREADS // 64)
    if red == "head":
        return dict(block=w // SK_COLS, lane=w % SK_COLS // 4, last=w // SK_COLS == (V - 1) // SK_COLS)
    if red == "lds":
        return dict(block=w // HO_BLK, wave=w % HO_BLK // 16, lane=w % 16 // 4, last=w // HO_BLK == (V - 1) // HO_BLK)
    kind, blk = red.rstrip("0123456789"), int(red[-2:])
    threads = FOLD_THREADS if kind == "fold" else FINISH_THREADS
    c = w // blk
    return dict(block=c, thread=c % threads, trip=c // threads, wave=c % threads // 64)


# reduction -> [(kind, chain, step)]: the pattern shown at `step` of the chain straddles the boundary `kind` of the
# reduction (test_cpu_greedy_tie_fixtures.py restates every kind as a predicate on locate() of the pair's two words).
# "adjacent_lanes" of the vector path is k VEC - 1 | k VEC inside a wave: 3 | 4 (fp32) and 15 | 16 (fp32 and bf16).
# The rows "k, k + 8192" / "k, k + 16384" of the heads' partials are the folds' same_thread claims.
CLAIMS = {
    "vec4": [("same_vector", "v16500_c", 6), ("adjacent_lanes", "v16500_a", 2), ("adjacent_lanes", "v16500_b", 1),
             ("adjacent_waves", "v16500_a", 3), ("next_load", "v16500_b", 5), ("next_pass", "v16500_c", 5),
             ("vector_tail", "v1003_a", 0), ("vector_tail", "v1003_b", 4), ("tail_alone", "v1003_a", 4),
             ("value_beats_index", "v16500_c", 2), ("value_beats_index", "v16500_c", 4),
             ("last_alone", "v16500_c", 0), ("first_ties_last", "v16500_a", 6)],
    "vec8": [("same_vector", "v16500_c", 6), ("adjacent_lanes", "v16500_a", 2), ("adjacent_waves", "v16500_a", 4),
             ("next_load", "v16500_b", 0), ("next_pass", "v16500_b", 2), ("vector_tail", "v16500_b", 4),
             ("vector_tail", "v1003_a", 0), ("tail_alone", "v16500_c", 0), ("tail_alone", "v1003_b", 0),
             ("value_beats_index", "v16500_c", 2), ("value_beats_index", "v16500_c", 4),
             ("last_alone", "v16500_c", 0), ("first_ties_last", "v16500_a", 6)],
    "scalar": [("adjacent_waves", "v16500_a", 1), ("wrap", "v16500_a", 3), ("same_thread", "v16500_a", 5),
               ("adjacent_waves", "v1003_a", 1), ("wrap", "v1003_a", 2), ("same_thread", "v1003_a", 3),
               ("value_beats_index", "v1003_a", 5), ("last_alone", "v1003_a", 4), ("first_ties_last", "v1003_b", 6)],
    "head": [("adjacent_lanes", "v16500_b", 1), ("adjacent_blocks", "v16500_b", 3), ("adjacent_blocks", "v16500_c", 1),
             ("ragged", "v1003_b", 5), ("value_beats_index", "v16500_c", 4), ("last_alone", "v16500_c", 0),
             ("last_alone", "v1003_a", 4), ("first_ties_last", "v16500_a", 6)],
    "lds": [("adjacent_lanes", "v16500_b", 1), ("adjacent_waves", "v16500_a", 2), ("adjacent_blocks", "v16500_a", 1),
            ("ragged", "v1003_b", 5), ("value_beats_index", "v16500_c", 4), ("last_alone", "v16500_c", 0),
            ("last_alone", "v1003_a", 4), ("first_ties_last", "v16500_a", 6)],
    "fold32": [("adjacent_lanes", "v16500_b", 3), ("adjacent_waves", "v16500_a", 0), ("wrap", "v16500_c", 1),
               ("same_thread", "v16500_c", 5), ("value_beats_index", "v16500_c", 2), ("last_alone", "v16500_c", 0),
               ("first_ties_last", "v16500_a", 6)],
    "fold64": [("adjacent_lanes", "v16500_a", 1), ("adjacent_waves", "v16500_c", 3), ("wrap", "v16500_d", 0),
               ("same_thread", "v16500_b", 2), ("value_beats_index", "v16500_c", 2), ("last_alone", "v16500_c", 0),
               ("first_ties_last", "v16500_a", 6)],
    # the finish kernel reduces the last step only: the claims sit at step steps - 1
    "finish32": [("wrap", "v16500_a", 7), ("same_thread", "v16500_b", 7)],
    "finish64": [("wrap", "v16500_d", 1), ("same_thread", "v16500_c", 7)],
}
# what every reduction's set must hold (the issue's table, by kind)
REQUIRED = {
    "vec4": {"same_vector", "adjacent_lanes", "adjacent_waves", "next_load", "next_pass", "vector_tail"},
    "vec8": {"same_vector", "adjacent_lanes", "adjacent_waves", "next_load", "next_pass", "vector_tail"},
    "scalar": {"adjacent_waves", "wrap", "same_thread"},
    "head": {"adjacent_lanes", "adjacent_blocks", "ragged"},
    "lds": {"adjacent_lanes", "adjacent_waves", "adjacent_blocks", "ragged"},
    "fold32": {"adjacent_lanes", "adjacent_waves", "wrap", "same_thread"},
    "fold64": {"adjacent_lanes", "adjacent_waves", "wrap", "same_thread"},
    "finish32": {"wrap", "same_thread"},
    "finish64": {"wrap", "same_thread"},
}
EVERY_SET = {"value_beats_index", "last_alone", "first_ties_last"}   # finish kernels excepted: one step per forward


# ---- device cases ---------------------------------------------------------------------------------------------------
# (form, dtype, E, B, mode); form "perop": Policy(greedy_step=1) for bf16 (fp32 is always per-op; so is B > 128);
# mode "greedy" / "select" / "sample" (sample(..., temperature=0)) / "eval" (greedy, eval(): the validation path)
CASES = (
    [("perop", dt, 512, B, m) for dt in ("fp32", "bf16") for B in (3, 129) for m in ("greedy", "select")]
    + [("perop", dt, 512, 3, "sample") for dt in ("fp32", "bf16")]
    + [("lds", "bf16", 512, B, "greedy") for B in (1, 33, 65, 128)]
    + [("lds", "bf16", 512, 33, "select"), ("lds", "bf16", 512, 3, "sample"), ("lds", "bf16", 512, 128, "sample"),
       ("lds", "bf16", 512, 3, "eval")]
    + [("skinny4", "bf16", 256, 3, "greedy"), ("skinny4", "bf16", 256, 65, "greedy")]
    + [("skinny8", "bf16", 1024, 3, "greedy"), ("skinny8", "bf16", 1024, 3, "sample")]
)
SIMPLE_CASES = (("perop", "fp32"), ("lds", "bf16"), ("perop", "bf16"))   # E = 512, B = 3, greedy


def form_of(dtype, E, B, perop_policy):
    """greedy_fused and the head selection (csrc/decoder.hip, csrc/skinny.hip) restated for a forward without teacher
    forcing: "perop", "lds", "skinny4" or "skinny8"."""
    fused = dtype == "bf16" and not perop_policy and 1 <= B <= 128 and E % 64 == 0 and 64 <= E <= 1024
    if not fused:
        return "perop"
    if E == 512:
        return "lds"
    return "skinny4" if E <= 512 else "skinny8"
