"""The VALUES of beam search on the device (Decoder.caption / caption_batch, csrc/beam.hip) in fp32 and bf16, at
real vocabularies, wide beams and exact ties.  Fixtures: beam_value_fixtures.py, qualified on the CPU by
test_cpu_beam_value_fixtures.py.  Every test needs an MI355X.

X  integer heads: ids equal and score == in both dtypes and both entry points; alpha rows within 1e-4 (fp32, the
   fp64 oracle) / 1e-2 (bf16, the fp64 beam-path mirror), the bounds test_gpu_parity / test_gpu_greedy hold.
F  fp32 at real sizes against the fp64 oracle: ids equal, alphas and score within 1e-4.
M  bf16 against the fp64 beam-path mirror on fit images: ids equal, alphas within 1e-2, the score within the preds
   rule summed over the path, 1e-2 * (sentence length) * (largest |logit| on the mirror's path).
Re-score: the returned ids fed back through a teacher-forced eval decoder of the same weights and dtype reproduce
   the returned alpha rows and, summed over the path, the returned score -- whatever the margins.

Measured on an MI355X (profiles/beam_values/new_gpu_tests.log): 63 passed in 13 s.  X: ids and score exact in every case, dtype
and entry point; alpha rows within 2.2e-7 (fp32) / 1.1e-5 (bf16).  F: alpha rows within 3.5e-8, score within 1.3e-6
of the fp64 oracle; re-scored alpha rows identical, score within 3.1e-6 (0.1 % of the bound).  M, paths of up to 51
steps: alpha rows within 2.1e-6 of the fp64 mirror, score within 1.1e-3 = 0.7 % of the bound at worst; re-scored
alpha rows within 2.9e-4, re-scored score within 23 % of its bound (the teacher-forced path stores bf16 logits, the
search fp32 ones).  Random weights at the COCO shape: 8 of 8 images completed (lengths 8 - 13) and re-scored, alpha
rows within 1.9e-7, score within 15 % of the bound.
"""
import math

import numpy as np
import pytest
import torch

import beam_value_fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda"
X = sorted(FX.X_CASES)
DTYPES = (torch.float32, torch.bfloat16)


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


@pytest.fixture(scope="module")
def decoder_of(sat):
    cache = {}

    def get(name, tf=False):
        if (name, tf) not in cache:
            c, p, _ = FX.load(name)
            kw = dict(tf=tf, ado=c["ado"], bert=c["bert"], attention=c["attention"])
            if c["bert"]:
                dec = sat.Decoder(c["V"], c["D"], bert_embedding_weight=p["embedding.weight"], **kw)
            else:
                dec = sat.Decoder(c["V"], c["D"], **kw)
            dec.load_state_dict(p, strict=True)
            cache[(name, tf)] = dec.to(DEV).eval()
        return cache[(name, tf)]
    return get


def rel(a, b):
    a = torch.as_tensor(np.asarray(a, dtype=np.float64)); b = torch.as_tensor(np.asarray(b, dtype=np.float64))
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def run(dec, c, feats, dtype, entry):
    """Per image (ids, alpha rows, score) from caption_batch or from caption (one call per image)."""
    f = feats.to(DEV).to(dtype)
    if entry == "batch":
        return [(ids, np.asarray(al, dtype=np.float64), s) for ids, al, s in
                dec.caption_batch(f, c["beam"], max_step=c["max_step"])]
    out = []
    for i in range(f.shape[0]):
        ids, al = dec.caption(f[i:i + 1].expand(c["beam"], c["L"], c["D"]).contiguous(), c["beam"],
                              max_step=c["max_step"])
        out.append((ids, np.asarray(al, dtype=np.float64), dec.last_caption_score))
    return out


def check_x(got, want, alpha_tol, tag):
    assert len(got) == len(want)
    worst = 0.0
    for i, ((ids, al, score), (e_ids, e_al, e_score, _)) in enumerate(zip(got, want)):
        assert ids == e_ids, (tag, i, ids, e_ids)
        assert score == e_score, (tag, i, score, e_score)          # integer sums: exact, -inf included
        assert al.shape == e_al.shape, (tag, i)
        worst = max(worst, rel(al, e_al))
    assert worst < alpha_tol, (tag, worst)
    return worst


# ---- X ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["batch", "single"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", X)
def test_x_exact_ids_and_score(decoder_of, name, dtype, entry):
    c, _, feats = FX.load(name)
    got = run(decoder_of(name), c, feats, dtype, entry)
    if dtype == torch.float32:
        worst = check_x(got, FX.expected(name, "f64"), 1e-4, (name, entry))
    else:
        worst = check_x(got, FX.expected(name, "m64"), 1e-2, (name, entry))
    print(f"X {name} {entry} {dtype}: alpha rel {worst:.2e}")
    assert len({tuple(g[0]) for g in got}) == 1                    # one head, other features: the same sentence


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["v10000_b17", "v1025_b64", "v4100_b33", "allneg_b5"])
def test_x_batch_order_does_not_matter(decoder_of, name, dtype):
    """One batch twice, the second time permuted: every image keeps its ids, score and alpha rows."""
    c, _, feats = FX.load(name)
    dec = decoder_of(name)
    perm = [2, 0, 1]
    a = run(dec, c, feats, dtype, "batch")
    b = run(dec, c, feats[perm].contiguous(), dtype, "batch")
    for j, src in enumerate(perm):
        assert b[j][0] == a[src][0] and b[j][2] == a[src][2]
        assert rel(b[j][1], a[src][1]) < (1e-4 if dtype == torch.float32 else 1e-2)


# ---- the re-score ---------------------------------------------------------------------------------------------------
def rescore(dec_tf, c, feats_row, dtype, ids, al, score, tag):
    """Feed the returned ids back as a caption, teacher-forced: the alpha rows and the summed gathered logits must be
    the search's.  Returns (alpha distance, score distance, score bound)."""
    n = len(ids)
    assert n >= 2
    pad = 0 if c["bert"] else 3
    caps = torch.tensor([ids + [pad] * (3 - n)] if n < 3 else [ids], dtype=torch.long, device=DEV)
    with torch.no_grad():
        preds, alphas = dec_tf(feats_row.to(DEV).to(dtype), caps)
    steps = n - 1                                  # a padded two-token result: step 1 only
    preds, alphas = preds[0, :steps].double().cpu(), alphas[0, :steps].double().cpu()
    tol = 1e-4 if dtype == torch.float32 else 1e-2
    d_al = rel(alphas.numpy(), al[1:])
    assert d_al < tol, (tag, d_al)
    logits = preds[torch.arange(steps), torch.tensor(ids[1:])]
    bound = tol * steps * logits.abs().max().item()
    d_sc = abs(logits.sum().item() - score)
    assert d_sc <= bound, (tag, d_sc, bound)
    return d_al, d_sc, bound


# ---- F ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["batch", "single"])
@pytest.mark.parametrize("name", FX.F_SETS)
def test_f_fp32_matches_fp64_oracle(decoder_of, name, entry):
    c, _, feats = FX.load(name)
    got = run(decoder_of(name), c, feats, torch.float32, entry)
    want = FX.expected(name, "f64")
    assert len(got) == len(want)
    for i, ((ids, al, score), (e_ids, e_al, e_score, _)) in enumerate(zip(got, want)):
        assert ids == e_ids, (name, i, ids, e_ids)
        assert al.shape == e_al.shape, (name, i)
        d_al = rel(al, e_al)
        assert d_al < 1e-4, (name, i, d_al)
        if math.isinf(e_score):
            assert math.isinf(score) and score < 0, (name, i)
            continue
        assert abs(score - e_score) <= 1e-4 * max(1.0, abs(e_score)), (name, i, score, e_score)
        r = rescore(decoder_of(name, tf=True), c, feats[i:i + 1], torch.float32, ids, al, score, (name, i))
        print(f"F {name}[{i}] {entry}: len {len(ids)} alpha rel {d_al:.2e} score err {abs(score - e_score):.2e}; "
              f"re-score alpha {r[0]:.2e} score {r[1]:.2e} (bound {r[2]:.2e})")


# ---- M ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["batch", "single"])
@pytest.mark.parametrize("name", FX.M_SETS)
def test_m_bf16_matches_fp64_mirror(decoder_of, name, entry):
    c, _, feats = FX.load(name)
    got = run(decoder_of(name), c, feats, torch.bfloat16, entry)
    want = FX.expected(name, "m64")
    assert len(got) == len(want)
    for i, ((ids, al, score), (e_ids, e_al, e_score, tr)) in enumerate(zip(got, want)):
        if i not in FX.m_images(name):      # an fp32-only image of the set
            continue
        assert ids == e_ids, (name, i, ids, e_ids)
        assert al.shape == e_al.shape, (name, i)
        d_al = rel(al, e_al)
        assert d_al < 1e-2, (name, i, d_al)
        if math.isinf(e_score):
            assert math.isinf(score) and score < 0, (name, i)
            continue
        bound = 1e-2 * (len(ids) - 1) * max(abs(x) for x in tr["path_logits"])
        d_sc = abs(score - e_score)
        r = rescore(decoder_of(name, tf=True), c, feats[i:i + 1], torch.bfloat16, ids, al, score, (name, i))
        print(f"M {name}[{i}] {entry}: len {len(ids)} alpha rel {d_al:.2e} score err {d_sc:.2e} (bound {bound:.2e}, "
              f"{d_sc / bound:.3f} of it); re-score alpha {r[0]:.2e} score {r[1]:.2e} (bound {r[2]:.2e})")
        assert d_sc <= bound, (name, i, d_sc, bound)


# ---- the random-weight bf16 COCO shape: no ids oracle, the re-score alone ----------------------------------------------
def test_bf16_coco_shape_rescored(sat):
    """test_bf16_coco_shape's decoder and features (its margins are inside bf16 noise, so no ids oracle): whatever
    the search picked, the teacher-forced decoder must reproduce its alpha rows and its score.  Randomly initialised
    weights never emit the end token, so its logit gets the bias the coco fixture set uses (there every one of 50
    oracle images then completed)."""
    torch.manual_seed(0)
    V, D, L, N, R = 10000, 2048, 49, 8, 3
    dec = sat.Decoder(V, D, ado=True, attention=True)
    with torch.no_grad():
        dec.f_out.bias[1] += FX.SETS["coco"]["eos_bias"]
    dec = dec.to(DEV).eval()
    feats = torch.randn(N, L, D, device=DEV).bfloat16()
    out = dec.caption_batch(feats, R, max_step=12)
    dec_tf = sat.Decoder(V, D, tf=True, ado=True, attention=True)
    dec_tf.load_state_dict({k: v.detach().cpu() for k, v in dec.state_dict().items()}, strict=True)
    dec_tf = dec_tf.to(DEV).eval()
    c = dict(bert=False)
    n_scored = 0
    for i, (ids, al, score) in enumerate(out):
        if math.isinf(score):
            continue
        r = rescore(dec_tf, c, feats[i:i + 1], torch.bfloat16, ids, np.asarray(al, dtype=np.float64), score, i)
        print(f"coco random[{i}]: len {len(ids)} re-score alpha {r[0]:.2e} score {r[1]:.2e} (bound {r[2]:.2e})")
        n_scored += 1
    print("re-scored", n_scored, "of", N)
    assert 2 * n_scored >= N
