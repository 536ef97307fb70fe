"""scst_weights on CPU tensors: w[b, t] = advantage[b] / B up to and including row b's first end token, 0 after it."""
import pytest
import torch

import sat_amd


def test_first_end_token_is_inclusive_and_later_steps_are_zero():
    sampled = torch.tensor([[5, 6, 1, 7, 1, 9],      # ends at t = 2; a second end token later changes nothing
                            [1, 4, 4, 4, 4, 4],      # ends at once: only step 0 is scored
                            [4, 5, 6, 7, 8, 1]],     # ends at the last step: every step is scored
                           dtype=torch.int32)
    adv = torch.tensor([1.5, -3.0, 0.75])
    w = sat_amd.scst_weights(sampled, adv, (1,))
    assert w.shape == sampled.shape and w.dtype == torch.float32 and w.is_contiguous()
    scored = torch.tensor([[1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=torch.bool)
    want = torch.where(scored, (adv / 3)[:, None], torch.zeros(()))
    assert torch.equal(w, want)
    assert bool((w[~scored] == 0).all())


def test_rows_without_an_end_token_get_all_steps():
    sampled = torch.tensor([[4, 5, 6, 7], [9, 9, 9, 9]], dtype=torch.int32)
    adv = torch.tensor([2.0, -1.0])
    w = sat_amd.scst_weights(sampled, adv, (1,))
    assert torch.equal(w, torch.tensor([[1.0] * 4, [-0.5] * 4]))


def test_bert_end_id_and_several_end_ids():
    sampled = torch.tensor([[2054, 102, 0, 0, 0], [2054, 2003, 2023, 102, 0]], dtype=torch.int32)
    adv = torch.tensor([1.0, 1.0])
    w = sat_amd.scst_weights(sampled, adv, (102,))
    assert torch.equal(w != 0, torch.tensor([[1, 1, 0, 0, 0], [1, 1, 1, 1, 0]], dtype=torch.bool))
    assert torch.equal(sat_amd.scst_weights(sampled, adv, 102), w)          # a bare id
    # the plain vocabulary's id 1 is an ordinary word here
    assert bool((sat_amd.scst_weights(sampled, adv, (1,)) != 0).all())
    both = sat_amd.scst_weights(sampled, adv, (102, 2003))
    assert torch.equal(both != 0, torch.tensor([[1, 1, 0, 0, 0], [1, 1, 0, 0, 0]], dtype=torch.bool))


def test_sign_and_scale():
    """The loss scores -logp = logsumexp - x_target per token, so the weight carries the advantage's own sign, scaled by
    1 / B: minimising sum w * (-logp) follows the policy gradient of E[advantage * logp] and raises the log-probability
    of rows with a positive advantage."""
    B = 8
    sampled = torch.full((B, 3), 7, dtype=torch.int32)
    adv = torch.linspace(-1.0, 1.0, B)
    w = sat_amd.scst_weights(sampled, adv, (1,))
    assert torch.equal(w, (adv / B)[:, None].expand(B, 3))
    assert bool((w[adv > 0] > 0).all()) and bool((w[adv < 0] < 0).all())
    # one gradient-descent step on sum w * (-logp) for a softmax policy: the drawn token's probability rises where
    # the advantage is positive and falls where it is negative
    logits = torch.zeros(B, 5, requires_grad=True)
    drawn = torch.arange(B) % 5
    logp = torch.log_softmax(logits, 1).gather(1, drawn[:, None]).squeeze(1)
    (w[:, 0] * -logp).sum().backward()
    after = torch.log_softmax(logits.detach() - 1.0 * logits.grad, 1).gather(1, drawn[:, None]).squeeze(1)
    assert bool((after[adv > 0] > logp.detach()[adv > 0]).all()) and bool((after[adv < 0] < logp.detach()[adv < 0]).all())


def test_shapes_are_checked():
    with pytest.raises(ValueError):
        sat_amd.scst_weights(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3), (1,))
    with pytest.raises(ValueError):
        sat_amd.scst_weights(torch.zeros(6, dtype=torch.int32), torch.zeros(6), (1,))


# ------------------------------------------------------------------ train.py --scst: flags and refusals
def _train_module():
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sat_train_cli_scst",
                                                  os.path.join(repo, "show-attend-and-tell_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_flags_and_refusals(capsys):
    T = _train_module()
    a = T.parse([])
    assert a.scst is False and a.scst_temperature == 1.0 and a.scst_reward == "cider"
    b = T.parse(["--scst", "--scst-temperature", "0.5", "--scst-reward", "bleu", "--cache-features",
                 "--fine-tune-encoder", "1", "--model", "m.pth"])
    assert (b.scst, b.scst_temperature, b.scst_reward, b.cache_features, b.fine_tune_encoder) == \
        (True, 0.5, "bleu", True, 1)
    assert set(vars(a)) == set(vars(b))
    for bad in (["--scst", "--tf"], ["--scst", "--tf-prob", "0.5"], ["--scst", "--scst-temperature", "-1"],
                ["--scst", "--scst-temperature", "nan"], ["--scst", "--scst-reward", "rouge"]):
        with pytest.raises(SystemExit):
            T.parse(bad)
    assert "cannot be combined with --tf" in " ".join(capsys.readouterr().err.split())   # a clear message
    for flag in ("--scst", "--scst-temperature", "--scst-reward"):
        assert flag in T.__doc__


def test_scst_reward_keys_references_by_image():
    """ScstReward on the host: the loader's all_captions only keys the references; both rewards give the reference
    itself the top score of its image."""
    import types
    T = _train_module()
    caps = torch.tensor([[0, 5, 6, 7, 8, 1, 3], [0, 6, 7, 9, 1, 3, 3], [0, 9, 8, 5, 4, 1, 3], [0, 4, 5, 9, 7, 6, 1]])
    ds = types.SimpleNamespace(caps=caps)
    for kind in ("cider", "bleu"):
        r = T.ScstReward(types.SimpleNamespace(bert=False, scst_reward=kind), ds)
        all_caps = caps[[2, 0]].unsqueeze(1).tolist()
        own = r([caps[2].tolist(), caps[0].tolist()], all_caps)
        other = r([caps[1].tolist(), caps[3].tolist()], all_caps)
        assert len(own) == 2 and all(isinstance(x, float) for x in own)
        assert own[0] > other[0] >= 0.0 and own[1] > other[1] >= 0.0
        assert r([[0, 1, 3, 3, 3, 3, 3]], all_caps[:1]) == [0.0]      # an empty caption
