"""The exact integer-valued cases (tests/exact_cases.py) checked on the CPU: every case of the table meets the
conditions its regime promises, every applicable wrong reference (a dropped product, truncation, round-half-away,
rounding before the residual add) differs from the true one -- so tests/test_gpu_exact.py would notice that fault in a
kernel -- and the bf16 rounding helper is torch's.  No GPU.
"""
import pytest
import torch

import exact_cases as X

IDS = [c.id for c in X.CASES]


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_table_names_every_family():
    assert set(X.FAMILIES) == {"gemm", "fast", "pipe", "stream", "chain", "proj", "ws", "stempool", "pool", "frag3x3",
                               "frag1x1", "block", "split", "skinny", "wgrad"}
    for fam in ("fast", "pipe", "stream", "chain", "proj", "ws", "stempool", "frag3x3", "frag1x1", "block"):
        regimes = {c.regime for c in X.CASES if c.family == fam and dict(c.p).get("cdt", X.BF) == X.BF}
        assert regimes == {"small", "rounding"}, fam   # bf16 output: both regimes


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_case_conditions_and_mutants(case):
    b = X.check_conditions(X.build(case, stats=True))
    if b.final is not None:
        print(X.figures(b))
    muts = X.applicable_mutants(b)
    if case.regime == "small":
        assert muts == ("drop",)
    elif case.regime == "rounding":
        assert muts[:2] == ("trunc", "away") and (len(muts) == 3) == (b.final["res"] is not None)
    for kind in muts:
        assert not _same(X.mutant(b, kind), b.outs), f"{case.id}: the {kind} mutant equals the reference"


def test_round_bf16_is_torch_rounding():
    """Round-to-nearest-even on a sweep with ties of both parities, both signs, and values next to the ties."""
    hi = torch.arange(0x3B80, 0x4780, dtype=torch.int64) << 16   # bf16 patterns 2^-8 .. 2^15, every mantissa
    lows = torch.tensor([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)
    bits = (hi[:, None] + lows[None, :]).reshape(-1)
    bits = torch.cat([bits, bits | (1 << 31)])
    bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
    v = bits.view(torch.float32)
    ties = X.is_tie(v)
    odd = ((bits.to(torch.int64) >> 16) & 1) == 1
    assert (ties & odd).any() and (ties & ~odd).any()
    assert torch.equal(X.round_bf16(v), v.bfloat16())
    assert torch.equal(X.round_bf16(v.double()), v.bfloat16())
    # the two wrong modes differ from it exactly where they should
    rne, away, trunc = X.round_bf16(v).float(), X.round_bf16(v, "away").float(), X.round_bf16(v, "trunc").float()
    assert torch.equal(away != rne, ties & ~odd)
    assert torch.equal(trunc != rne, ((bits.to(torch.int64) & 0xFFFF) > 0x8000) | (ties & odd))
    assert (trunc.abs() <= v.abs()).all()


def test_generators_are_reproducible():
    a, b = X.ints(X._gen("t", 1), (64,), 5), X.ints(X._gen("t", 1), (64,), 5)
    assert torch.equal(a, b) and a.abs().max() <= 5 and torch.equal(a, a.round())
    t = X.ternary(X._gen("t", 2), (4096,), 0.25)
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.2 < t.abs().mean() < 0.3
