"""The greedy tie fixtures (greedy_tie_fixtures.py) qualified with the oracle alone.  No GPU.

Exactness: the fp32, fp64 and bf16-mirror oracle return the same integer logits and the hand-derived tokens, with and
without the dropout mask.  Well-formed chains.  Boundaries: every claim recomputed from V, the block sizes and the
dtype.  And the planted patterns fail under the wrong rules: every pair changes its winner under "the higher index",
every value-beats-index pattern under "the first word at or above the runner-up"."""
import numpy as np
import pytest
import torch

import greedy_tie_fixtures as FX
from oracle import sat_oracle as O

CHAINS = sorted(FX.CHAINS)
E = 512


def _oracle(p, feats, caps, dtype, mirror, masks, tf=False, ado=True):
    q = {k: v.to(dtype) for k, v in p.items()}
    kw = dict(tf=tf, ado=ado, attention=True, training=masks is not None,
              dropout_masks=None if masks is None else masks.to(dtype))
    with torch.no_grad():
        if mirror:
            with O.bf16_mirror():
                return O.decoder_forward(q, feats.to(dtype), caps, **kw)
        return O.decoder_forward(q, feats.to(dtype), caps, **kw)


ARITHMETICS = (("fp32", torch.float32, False), ("fp64", torch.float64, False), ("mirror", torch.float64, True))


# ---- exactness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
def test_chain_is_exact_in_every_arithmetic(name):
    c = FX.chain(name)
    B, T1 = 3, c["steps"]
    p, feats, caps = FX.chain_params(name, E), FX.features(B), FX.plain_captions(B, T1)
    e = FX.expected(name, B)
    want = FX.expected_preds(name, e["shown"])
    assert torch.equal(e["tokens"], torch.tensor(c["tokens"]).expand(B, T1))
    alphas = []
    for tag, dtype, mirror in ARITHMETICS:
        for masks in (FX.dropout_masks(B, T1, E), None):   # the mask is irrelevant to the logits by construction
            preds, al, tokens = _oracle(p, feats, caps, dtype, mirror, masks)
            assert torch.equal(preds.float(), want), (tag, masks is None)
            assert torch.equal(tokens, e["tokens"]), (tag, masks is None)
            assert torch.equal(preds.argmax(2), e["win"]), tag   # the last step's winner too (the sample form)
        alphas.append(al)
    # h and the alphas are ordinary numbers: the rows differ, and so do the arithmetics
    assert (alphas[1][0] - alphas[1][1]).abs().max() > 1e-6
    assert 0 < (alphas[2] - alphas[1]).abs().max() < 2e-2


@pytest.mark.parametrize("name", CHAINS)
def test_chain_is_well_formed(name):
    c = FX.chain(name)
    V, n = c["V"], c["n"]
    assert n <= 8 and 2 <= c["steps"] <= 8
    assert np.array_equal(c["vectors"], np.round(c["vectors"])) and np.abs(c["vectors"]).max() <= 64
    assert len(set(c["winners"])) == n                       # no winner is shared by two patterns
    assert 0 not in c["winners"][:-1]                        # token 0 is the start token: such a pattern goes last
    assert c["pat"][0] == 0 and c["shown"][:n] == list(range(n))   # every pattern is reached, in order
    for k, w in enumerate(c["winners"][:-1]):
        assert c["pat"][w] == k + 1
    assert c["pat"].min() == 0 and c["pat"].max() == n - 1
    if c["steps"] == n + 1:                                   # the wrap: the last winner is a fed token
        assert c["tokens"][n] == c["winners"][-1] and c["shown"][n] == c["pat"][c["winners"][-1]]
    for spec, w in zip(c["patterns"], c["winners"]):          # the winners, by hand
        assert w == (0 if spec == FX.ALLNEG else spec[1]), spec   # pair: i; top, vbi: the top word; all zeros: 0


# ---- the wrong rules ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
def test_patterns_fail_under_the_wrong_rules(name):
    c = FX.chain(name)
    kinds = set()
    for spec, v in zip(c["patterns"], np.maximum(c["vectors"], 0.0)):
        kinds.add(spec[0])
        if spec[0] in ("pair", "allneg"):    # decided by the index rule
            assert FX.winner(v, "higher") != FX.winner(v), spec
            assert (v == v.max()).sum() >= 2
        if spec[0] == "pair":
            assert (v == v.max()).sum() == 2 and FX.winner(v, "higher") == spec[2]
            assert np.sort(np.unique(v))[-2] > v.min()        # a lower plateau elsewhere
        if spec[0] in ("vbi", "top"):        # decided by the value: the index must not beat it
            assert FX.winner(v, "first_ge") != FX.winner(v), spec
            assert FX.winner(v, "first_ge") < FX.winner(v) and (v == v.max()).sum() == 1
            assert FX.winner(v, "higher") == FX.winner(v)
    assert "pair" in kinds


def test_winner_restates_torch_argmax():
    rng = np.random.default_rng(5)
    for _ in range(50):
        x = rng.integers(-3, 4, size=37).astype(np.float64)
        assert FX.winner(x) == int(torch.from_numpy(x).argmax())
        assert FX.winner(x, "higher") == 36 - int(torch.from_numpy(x[::-1].copy()).argmax())
    x = np.array([FX.INF, FX.NAN, 1.0, FX.NAN])
    assert FX.winner(x) == 1 and FX.winner(x, "higher") == 3


# ---- boundaries -----------------------------------------------------------------------------------------------------
def _unit(red, a, b):
    """Two words in one lane / thread of the reduction."""
    if red in ("head", "lds"):
        return a["block"] == b["block"] and a["lane"] == b["lane"] and a.get("wave") == b.get("wave")
    if red.startswith("vec"):
        return not a["tail"] and not b["tail"] and a["thread"] == b["thread"]
    return a["thread"] == b["thread"]


def _vec(kind, a, b, i, j):
    if kind == "vector_tail":
        return not a["tail"] and b["tail"]
    if a["tail"] or b["tail"]:
        return False
    return {"same_vector": a["vector"] == b["vector"],
            "adjacent_lanes": j == i + 1 and (a["trip"], a["load"], a["wave"]) == (b["trip"], b["load"], b["wave"])
            and b["thread"] == a["thread"] + 1,
            "adjacent_waves": j == i + 1 and (a["trip"], a["load"]) == (b["trip"], b["load"])
            and a["thread"] % 64 == 63 and b["thread"] == a["thread"] + 1,
            "next_load": (a["trip"], a["thread"]) == (b["trip"], b["thread"]) and b["load"] == a["load"] + 1,
            "next_pass": (a["thread"], a["load"]) == (b["thread"], b["load"]) and b["trip"] == a["trip"] + 1}[kind]


def _threads(kind, a, b, i, j, threads, blocks):
    """scalar path (blocks = False: one word per trip and thread) and the folds (blocks: one partial)."""
    step = b["block"] == a["block"] + 1 if blocks else j == i + 1
    return {"adjacent_lanes": step and a["trip"] == b["trip"] and a["wave"] == b["wave"]
            and b["thread"] == a["thread"] + 1,
            "adjacent_waves": step and a["trip"] == b["trip"] and a["thread"] % 64 == 63
            and b["thread"] == a["thread"] + 1,
            "wrap": step and a["thread"] == threads - 1 and b["thread"] == 0 and b["trip"] == a["trip"] + 1,
            "same_thread": a["thread"] == b["thread"] and b["trip"] > a["trip"]}[kind]


def _head(red, kind, a, b, i, j, V):
    blk = FX.SK_COLS if red == "head" else FX.HO_BLK
    if kind == "ragged":   # the winner inside a partial last block; the skinny head's scalar store path: V % 4 != 0
        return V % blk != 0 and a["last"] and b["last"] and (red == "lds" or V % 4 != 0)
    if kind == "adjacent_blocks":
        return j == i + 1 and b["block"] == a["block"] + 1
    same = a["block"] == b["block"]
    if kind == "adjacent_waves":
        return red == "lds" and same and j == i + 1 and b["wave"] == a["wave"] + 1
    return kind == "adjacent_lanes" and same and j == i + 1 and a.get("wave") == b.get("wave") \
        and b["lane"] == a["lane"] + 1


def _holds(red, kind, spec, V):
    if kind == "last_alone":
        return spec == FX.top(V - 1)
    if kind == "first_ties_last":
        return spec == FX.pair(0, V - 1)
    if kind == "tail_alone":
        return spec[0] == "top" and FX.locate(red, spec[1], V)["tail"]
    if kind == "value_beats_index":
        w = FX.locate(red, spec[1], V) if spec[0] == "vbi" else None
        return w is not None and all(lo < spec[1] for lo in spec[2]) and \
            any(_unit(red, FX.locate(red, lo, V), w) for lo in spec[2])
    if spec[0] != "pair":
        return False
    i, j = spec[1], spec[2]
    a, b = FX.locate(red, i, V), FX.locate(red, j, V)
    if red.startswith("vec"):
        return _vec(kind, a, b, i, j)
    if red == "scalar":
        return _threads(kind, a, b, i, j, FX.AM_THREADS, False)
    if red in ("head", "lds"):
        return _head(red, kind, a, b, i, j, V)
    return _threads(kind, a, b, i, j, FX.FOLD_THREADS if red.startswith("fold") else FX.FINISH_THREADS, True)


BOUNDARY = [(red, kind, name, step) for red, claims in FX.CLAIMS.items() for kind, name, step in claims]


@pytest.mark.parametrize("red,kind,name,step", BOUNDARY, ids=[f"{r}-{k}-{n}-{s}" for r, k, n, s in BOUNDARY])
def test_claimed_boundary_is_straddled(red, kind, name, step):
    c = FX.chain(name)
    V, T1 = c["V"], c["steps"]
    spec = c["patterns"][c["shown"][step]]
    assert _holds(red, kind, spec, V), (spec, red, kind)
    if red.startswith("finish"):
        assert step == T1 - 1            # the finish kernel reduces the last step
    else:
        assert step < T1 - 1             # a greedy forward reduces this step: its winner is the next fed token
    # the per-op path the step takes, from the row pointers' alignment
    if red == "vec4":
        assert FX.perop_path(V, T1, step, 4) == "vector"
    if red == "vec8":
        assert FX.perop_path(V, T1, step, 2) == "vector"
    if red == "scalar":
        assert "scalar" in (FX.perop_path(V, T1, step, 2), FX.perop_path(V, T1, step, 4))
    # the second trips exist: more partials than the fold has threads
    if kind in ("wrap", "same_thread") and red[:4] in ("fold", "fini"):
        blk = int(red[-2:])
        ncb = FX.head_blocks(V, 512 if blk == 64 else 256)
        assert ncb == -(-V // blk) and ncb > (FX.FOLD_THREADS if red.startswith("fold") else FX.FINISH_THREADS)


def test_every_reduction_has_its_set():
    assert sorted(FX.CLAIMS) == sorted(FX.REQUIRED)
    for red, claims in FX.CLAIMS.items():
        kinds = {k for k, _, _ in claims}
        need = FX.REQUIRED[red] | (set() if red.startswith("finish") else FX.EVERY_SET)
        assert need <= kinds, (red, need - kinds)
    # the fold thresholds: a second trip above 256 partials
    assert FX.head_blocks(16384, 512) == 256 and FX.head_blocks(16385, 512) == 257
    assert FX.head_blocks(8192, 256) == 256 and FX.head_blocks(8193, 1024) == 257
    assert FX.head_blocks(16500, 512) == 258 and FX.head_blocks(16500, 256) == 516


def test_both_perop_paths_occur_for_each_dtype():
    for esz in (4, 2):
        paths = {FX.perop_path(FX.chain(n)["V"], FX.chain(n)["steps"], t, esz)
                 for n in CHAINS for t in range(FX.chain(n)["steps"] - 1)}
        assert paths == {"vector", "scalar"}, esz
        simple = {FX.perop_path(V, T1, t, esz) for V, T1 in FX.SIMPLE_STEPS.items() for t in range(T1 - 1)}
        assert simple == {"vector", "scalar"}, esz
    assert FX.perop_paths("v16500_a", 2) == ["vector", "scalar"] * 4
    assert FX.perop_paths("v16500_d", 2) == ["vector", "scalar"]
    assert FX.perop_paths("v1003_a", 4) == ["vector", "scalar", "scalar", "scalar"] * 2
    # what the module docstring says of the two vocabularies
    assert [FX.perop_path(16500, 8, t, 2) for t in range(4)] == ["vector", "scalar", "vector", "scalar"]
    assert {FX.perop_path(16500, 8, t, 4) for t in range(8)} == {"vector"}
    assert [t for t in range(8) if FX.perop_path(1003, 8, t, 4) == "vector"] == [0, 4]
    assert [t for t in range(8) if FX.perop_path(1003, 8, t, 2) == "vector"] == [0]
    assert {FX.perop_path(1003, 5, t, e) for t in range(5) for e in (2, 4)} == {"scalar"}


# ---- the select form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
def test_select_rows_show_different_patterns(name):
    c = FX.chain(name)
    T1, n = c["steps"], c["n"]
    for B in (3, 33, 129):
        caps, keep = FX.select_inputs(name, B)
        e = FX.expected(name, B, select=True)
        k = keep[:, 1:].bool()
        assert bool(keep[:, 0].all()) and 0 < int(k.sum()) < k.numel()
        assert not set(caps[:, 1:T1][k].tolist()) & set(c["winners"])      # a kept token is no pattern's winner
        assert torch.equal(e["tokens"][:, 1:][k], caps[:, 1:T1][k])
        prev_win = e["win"][:, :-1]
        assert torch.equal(e["tokens"][:, 1:][~k], prev_win[~k])
        # the rows of one 16-row fragment: at some step at least three patterns with three winners (all of B = 3's rows)
        rows = min(B, 16)
        most = max(len({(int(s), int(w)) for s, w in zip(e["shown"][:rows, t], e["win"][:rows, t])})
                   for t in range(1, T1 - 1 if T1 > 2 else T1))
        if n >= 3:
            assert most >= 3 and len(set(e["win"][:rows].flatten().tolist())) >= 3, (B, most)
        else:
            assert most == 2
    # the oracle fed the restated tokens returns the predicted logits, whose argmax is the next winner
    B = 3
    e = FX.expected(name, B, select=True)
    fed = FX.plain_captions(B, T1)
    fed[:, :T1] = e["tokens"]
    for tag, dtype, mirror in ARITHMETICS:
        preds, _, tokens = _oracle(FX.chain_params(name, E), FX.features(B), fed, dtype, mirror,
                                   FX.dropout_masks(B, T1, E), tf=True)
        assert torch.equal(preds.float(), FX.expected_preds(name, e["shown"])), tag
        assert torch.equal(preds.argmax(2), e["win"]) and torch.equal(tokens, e["tokens"]), tag


# ---- the simple head ------------------------------------------------------------------------------------------------
SIMPLE_WINNERS = {"pair_63_64": lambda V: 63, "last_alone": lambda V: V - 1, "nan_behind_inf": lambda V: 200,
                  "all_minus_inf": lambda V: 0, "two_inf": lambda V: 70}


@pytest.mark.parametrize("V", FX.SIMPLE_V)
@pytest.mark.parametrize("name", sorted(FX.SIMPLE_PATTERNS))
def test_simple_pattern(name, V):
    x = FX.simple_vector(name, V)
    w = SIMPLE_WINNERS[name](V)
    assert FX.winner(x) == w
    t = torch.from_numpy(x)
    for dt in (torch.float32, torch.float64, torch.bfloat16):   # what torch's max(1)[1] does with it (decoder.py:132)
        assert int(t.to(dt).unsqueeze(0).max(1)[1]) == w, dt
        assert torch.equal(t.to(dt).double().nan_to_num(nan=7.5), t.nan_to_num(nan=7.5))   # exact in every format
    if name in ("pair_63_64", "two_inf", "nan_behind_inf"):
        assert FX.winner(x, "higher") != w
    if V != 1003:
        return
    B, T1 = 3, FX.SIMPLE_STEPS[V]
    p = FX.simple_params(name, V, E)
    for tag, dtype, mirror in ARITHMETICS:
        for masks in (FX.dropout_masks(B, T1, E), None):
            preds, _, tokens = _oracle(p, FX.features(B), FX.plain_captions(B, T1), dtype, mirror, masks, ado=False)
            want = t.float().expand(B, T1, V)
            assert torch.equal(torch.isnan(preds), torch.isnan(want)), tag
            assert torch.equal(preds.float().nan_to_num(nan=7.5), want.nan_to_num(nan=7.5)), tag
            assert torch.equal(tokens, torch.tensor([0] + [w] * (T1 - 1)).expand(B, T1)), tag


# ---- the device cases -----------------------------------------------------------------------------------------------
def test_cases_name_their_forms():
    forms = set()
    for form, dt, E_, B, mode in FX.CASES:
        assert FX.form_of(dt, E_, B, perop_policy=form == "perop") == form, (form, dt, E_, B)
        forms.add((form, mode))
    assert FX.form_of("bf16", 512, 129, False) == "perop"      # B > 128: the per-op step without the policy
    # every batch class of the LDS head (MB = 2 / 4 / 8 for B <= 32 / 64 / 128), rows past B clamped
    assert {(B > 32) + (B > 64) for f, _, _, B, m in FX.CASES if f == "lds" and m == "greedy"} == {0, 1, 2}
    assert all(B % 16 for f, _, _, B, m in FX.CASES if f == "lds" and m == "greedy" and B < 128)
    for form in ("perop", "lds"):
        assert {(form, m) for m in ("greedy", "select", "sample")} <= forms
    assert {("skinny4", "greedy"), ("skinny8", "greedy"), ("skinny8", "sample"), ("lds", "eval")} <= forms
    assert [FX.form_of(dt, 512, 3, f == "perop") for f, dt in FX.SIMPLE_CASES] == [f for f, _ in FX.SIMPLE_CASES]
