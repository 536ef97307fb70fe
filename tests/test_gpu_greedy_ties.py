"""The greedy feedback argmax on planted exact ties, in every kernel form (fixtures: greedy_tie_fixtures.py, qualified
on the host by test_cpu_greedy_tie_fixtures.py).

Forms: the per-op step (``argmax_kernel``: fp32, bf16 under Policy(greedy_step=1), B > 128), the fused bf16 step with
the LDS-staged head (E = 512: ``head_out_lds_kernel``) and with the skinny head (E = 256: 4 waves, E = 1024: 8 waves;
``head_out_kernel``), each followed by the LSTM kernel's token fold; plain greedy, the select form (scheduled sampling
under an injected keep mask), ``sample`` at temperature 0 (``sampled_finish_kernel`` reduces the last step on the
fused path) and one eval() case.  The simple head carries the non-finite patterns.

Every compared quantity is an exact integer, NaN or +-inf: tokens and logits are compared with ``==``, so a wrong token
is never excused by a wrong logit, nor the reverse.  No tolerance appears anywhere.
"""
import ctypes

import pytest
import torch

import greedy_tie_fixtures as FX
import test_gpu_sched_sampling as SS
import test_gpu_shapes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


_DECODERS = {}


def _decoder(sat, p, V, E, ado):
    """One module per (V, E, head), shared: a case loads its weights into it and sets every switch it reads."""
    key = (V, E, ado)
    if key not in _DECODERS:
        _DECODERS[key] = SS._decoder(sat, dict(bert=False, tf=False, att=True, ado=ado, E=E, D=FX.D, V=V, p=p))
    dec = _DECODERS[key]
    dec.load_state_dict(p, strict=True)
    dec.policy = dec.tf_prob = dec.tf_mask = dec.dropout_mask = None
    dec.split_target = 0
    return dec


def _workspace_bytes(sat, dec, feats, caps):
    L = sat._lib
    return L.lib().sat_decoder_workspace_bytes(ctypes.byref(dec._dims(feats, caps)))


def _assert_form(sat, dec, feats, caps, form, dt, E, B):
    """The case ran the form it names: the instance, greedy_fused's conditions restated (FX.form_of), and the fused
    step's own workspace regions (the token table, the argmax partials) present exactly when the step is fused."""
    inst = S._instance(sat, dec, feats, caps)
    assert inst["fwd_launches_per_step"] == 4 and inst["bwd_launches_per_step"] == 4, inst
    if dt == "bf16":
        assert inst["transposed"] == 1, inst
    perop_policy = dec.policy is not None
    assert FX.form_of(dt, E, B, perop_policy) == form
    own = _workspace_bytes(sat, dec, feats, caps)
    policy, dec.policy = dec.policy, sat.Policy(greedy_step=1)
    try:
        perop = _workspace_bytes(sat, dec, feats, caps)
    finally:
        dec.policy = policy
    assert own > 0 and perop > 0 and (own > perop) == (form != "perop"), (own, perop, form)


def _forward(sat, dec, form, dt, E, B, mode, T1, caps, keep=None):
    """One forward of a prepared module; returns what the tests compare, on the device."""
    dtype = DTYPES[dt]
    if form == "perop" and dt == "bf16" and B <= 128:
        dec.policy = sat.Policy(greedy_step=1)
    if mode == "eval":
        dec.eval()
    else:
        dec.train()
        dec.dropout_mask = FX.dropout_masks(B, T1, E).permute(1, 0, 2).contiguous().to(torch.uint8)
    if mode == "select":
        dec.tf_prob, dec.tf_mask = 0.5, keep.clone()
    feats = FX.features(B).to(DEV).to(dtype)
    caps = caps.to(DEV)
    sampled = None
    with torch.no_grad():
        if mode == "sample":
            preds, _, sampled = dec.sample(feats, T1, temperature=0.0)
        else:
            preds, _ = dec(feats, caps)
    torch.cuda.synchronize()
    _assert_form(sat, dec, feats, caps, form, dt, E, B)
    assert preds.dtype == dtype and tuple(preds.shape) == (B, T1, dec.vocabulary_size)
    return dict(preds=preds.float(), tokens=dec.last_tokens.long().cpu(),
                sampled=None if sampled is None else sampled.long().cpu(),
                keep=None if dec.last_tf_mask is None else dec.last_tf_mask.cpu())


def _same(a, b):
    """torch.equal with NaN compared by position."""
    na, nb = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros((), dtype=a.dtype, device=a.device)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


CHAIN_CASES = [(case, name) for case in FX.CASES for name in FX.CHAINS]


@pytest.mark.parametrize("case,name", CHAIN_CASES, ids=["-".join(map(str, c)) + "-" + n for c, n in CHAIN_CASES])
def test_chain(sat, case, name):
    form, dt, E, B, mode = case
    c = FX.chain(name)
    T1 = c["steps"]
    select = mode == "select"
    caps, keep = FX.select_inputs(name, B) if select else (FX.plain_captions(B, T1), None)
    dec = _decoder(sat, FX.chain_params(name, E), c["V"], E, True)
    h = _forward(sat, dec, form, dt, E, B, mode, T1, caps, keep)
    e = FX.expected(name, B, select=select)
    print(f"GREEDYTIE {form} {dt} E={E} B={B} {mode} {name}: row 0 fed {h['tokens'][0].tolist()}")
    # the fed tokens: the hand-derived chain; under the select form the host restatement (FX.expected)
    assert torch.equal(h["tokens"], e["tokens"]), (h["tokens"] != e["tokens"]).nonzero()[:8].tolist()
    # the logits: the integer pattern every row shows
    want = FX.expected_preds(name, e["shown"]).to(DEV)
    assert torch.equal(h["preds"], want), (h["preds"] != want).nonzero()[:8].tolist()
    if select:
        assert torch.equal(h["keep"], keep)
        assert torch.equal(h["tokens"][:, 1:][keep[:, 1:].bool()], caps[:, 1:T1][keep[:, 1:].bool()])
    else:
        assert h["keep"] is None
        assert torch.equal(h["tokens"], h["tokens"][:1].expand(B, T1))      # every row equals row 0
        assert torch.equal(h["preds"], h["preds"][:1].expand(B, T1, c["V"]))
    if mode == "sample":   # the draw at temperature 0 is the winner of every step, the last included
        assert torch.equal(h["sampled"], e["win"]), (h["sampled"] != e["win"]).nonzero()[:8].tolist()
        assert torch.equal(h["sampled"][:, :-1], h["tokens"][:, 1:])


SIMPLE = [(f, dt, n, V) for f, dt in FX.SIMPLE_CASES for n in FX.SIMPLE_PATTERNS for V in FX.SIMPLE_V]


@pytest.mark.parametrize("form,dt,name,V", SIMPLE, ids=[f"{f}-{dt}-{n}-v{V}" for f, dt, n, V in SIMPLE])
def test_simple_head(sat, form, dt, name, V):
    E, B, T1 = 512, 3, FX.SIMPLE_STEPS[V]
    x = FX.simple_vector(name, V)
    w = FX.winner(x)
    dec = _decoder(sat, FX.simple_params(name, V, E), V, E, False)
    h = _forward(sat, dec, form, dt, E, B, "greedy", T1, FX.plain_captions(B, T1))
    print(f"GREEDYTIE simple {form} {dt} V={V} {name}: row 0 fed {h['tokens'][0].tolist()}")
    assert torch.equal(h["tokens"], torch.tensor([0] + [w] * (T1 - 1)).expand(B, T1))
    want = torch.from_numpy(x).float().to(DEV).expand(B, T1, V)
    assert _same(h["preds"], want)
