"""The joint planner of the grouped split-K GEMM launch (csrc/gemmsplit.hip plan_group, through the host-only C
entries sat_gemm_group_plan / sat_gemm_group_block), without a GPU.

The sets: the benchmark's three groups of the decoder backward (B = 128, T = 27, V = 10000, E = 512, D = 2048,
L = 49), the small products of tests/test_gpu_gemm_group.py, forced plans, and sets that cannot fit their workspace.
For every planned set: each (product, tile, split) has exactly one block and each block maps back to it; the slab
regions and ticket ranges of the split products are disjoint and inside the buffers; every split has at least two
k-tiles and none is empty; a product whose forced split cannot be held is reported as falling back, never clipped.
"""
import pytest

SLAB = 256 * 256 * 128 * 4      # the partial-tile bytes of sat_gemm_workspace_bytes()
TICKETS = 1024
R, V, E, D, L, B = 3328, 10000, 512, 2048, 49, 128
HG = 5 * E + D

SETS = {
    "head pair": [(V, E, R), (R, E, V)],
    "head four": [(E, E, R), (E, D, R), (R, E, E), (R, D, E)],
    "after the loop": [(E, D, B * L), (HG, E, R), (4 * E, E, R), (4 * E, D, R), (R, E, 4 * E)],
    "small, forced": [(264, 136, 328, 128, 2), (128, 128, 64, 128, 1), (8, 8, 8, 128, 1)],
    "small, 256 rows": [(264, 136, 328, 256, 2), (128, 128, 64, 256, 1), (8, 8, 8, 256, 1)],
    "more blocks than CUs": [(2560, 2048, 128, 128, 1), (264, 136, 328, 128, 2)],
    "free small": [(264, 136, 328), (128, 128, 64), (8, 8, 8)],
    "forced splits everywhere": [(512, 512, 3328, 128, 8), (2048, 512, 3328, 256, 4), (1024, 512, 2048, 128, 3)],
}


@pytest.fixture(scope="module")
def ops():
    from sat_amd import ops
    return ops


def check_plan(ops, shapes, plan, slab, tickets):
    nblocks = 0
    regions, ranges = [], []
    for sh, p in zip(shapes, plan):
        if p.fallback:
            assert p.blocks == 0
            continue
        M, N, K = sh[:3]
        assert p.tile_rows in (128, 256)
        if len(sh) > 3 and sh[3]:
            assert p.tile_rows == sh[3]
        if len(sh) > 4 and sh[4]:
            assert p.splits == sh[4]
        assert p.tiles_m == -(-M // p.tile_rows) and p.tiles_n == -(-N // 128)
        assert p.blocks == p.tiles_m * p.tiles_n * p.splits
        # K ranges [s kchunk, min(K, (s + 1) kchunk)): whole 64-deep k-tiles, none empty, >= 2 k-tiles when split
        assert 1 <= p.splits <= 8 and p.kchunk % 64 == 0
        assert (p.splits - 1) * p.kchunk < K <= p.splits * p.kchunk
        if p.splits > 1:
            nk = -(-K // 64)
            assert nk >= 2 * p.splits
            for s in range(p.splits):
                kt = -(-(min(K, (s + 1) * p.kchunk) - s * p.kchunk) // 64)
                assert kt >= 2
            assert p.slab_bytes == p.blocks * p.tile_rows * 128 * 4 and p.tickets == p.tiles_m * p.tiles_n
            regions.append((p.slab_offset, p.slab_offset + p.slab_bytes))
            ranges.append((p.ticket_offset, p.ticket_offset + p.tickets))
        nblocks += p.blocks
    for spans, cap in ((regions, slab), (ranges, tickets)):
        spans.sort()
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 <= b0
        assert all(0 <= a0 < a1 <= cap for a0, a1 in spans)
    # blocks <-> work items, one to one; the products' block ranges tile [0, nblocks)
    seen = set()
    for b in range(nblocks):
        i, mt, nt, s = ops.gemm_group_block(plan, b)
        p = plan[i]
        assert i >= 0 and not p.fallback and p.first_block <= b < p.first_block + p.blocks
        assert 0 <= mt < p.tiles_m and 0 <= nt < p.tiles_n and 0 <= s < p.splits
        seen.add((i, mt, nt, s))
    assert len(seen) == nblocks
    assert ops.gemm_group_block(plan, nblocks)[0] == -1 and ops.gemm_group_block(plan, -1)[0] == -1
    return nblocks


@pytest.mark.parametrize("name", list(SETS))
def test_planned_set_is_consistent(ops, name):
    shapes = SETS[name]
    plan = ops.gemm_group_plan(shapes, SLAB, TICKETS)
    assert not any(p.fallback for p in plan)
    check_plan(ops, shapes, plan, SLAB, TICKETS)
    # deterministic: the same set plans the same way
    again = ops.gemm_group_plan(shapes, SLAB, TICKETS)
    assert [bytes(a) for a in again] == [bytes(p) for p in plan]


def test_long_items_come_first(ops):
    """Block order: products by their longest work item, so a long item never starts in the last round."""
    for name in ("head pair", "head four", "after the loop"):
        plan = ops.gemm_group_plan(SETS[name], SLAB, TICKETS)
        by_block = sorted(plan, key=lambda p: p.first_block)
        cost = [(p.kchunk // 64) * (1.10 if p.tile_rows == 256 else 0.73) for p in by_block]
        assert cost == sorted(cost, reverse=True), (name, cost)


def test_many_rounds_allowed(ops):
    """tiles x splits may pass the 256 CUs of one round: the last arriver never waits for another workgroup."""
    plan = ops.gemm_group_plan([(2048, 2048, 3328, 128, 2), (4608, 512, 3328, 128, 1)], SLAB, TICKETS)
    assert plan[0].splits == 2 and plan[0].blocks == 512 and not plan[0].fallback
    check_plan(ops, [(2048, 2048, 3328, 128, 2), (4608, 512, 3328, 128, 1)], plan, SLAB, TICKETS)


def test_forced_split_that_cannot_fit_falls_back(ops):
    """Forced split counts whose regions pass the slab bytes or the tickets: the product is reported as falling back
    (its own launch), the others still plan, and nothing is clipped to fit."""
    shapes = [(2048, 2048, 3328, 128, 2), (2048, 2048, 3328, 128, 2), (264, 136, 328, 128, 2)]
    plan = ops.gemm_group_plan(shapes, SLAB, TICKETS)   # 32 MiB each: the second one has no room
    assert [p.fallback for p in plan] == [0, 1, 1]
    check_plan(ops, shapes, plan, SLAB, TICKETS)
    plan = ops.gemm_group_plan(shapes, SLAB, 16)        # 256 tiles need 256 tickets
    assert [p.fallback for p in plan] == [1, 1, 0]
    check_plan(ops, shapes, plan, SLAB, 16)
    plan = ops.gemm_group_plan(shapes, 0, 0)            # no workspace at all
    assert [p.fallback for p in plan] == [1, 1, 1]
    # a split count the K range cannot hold (one k-tile): as for a single launch, not this kernel's
    plan = ops.gemm_group_plan([(128, 128, 64, 128, 2), (128, 128, 640, 128, 2)], SLAB, TICKETS)
    assert [p.fallback for p in plan] == [1, 0]


def test_free_products_run_unsplit_without_workspace(ops):
    """Without slab bytes or tickets the planner may still group: every free product unsplit, none falling back."""
    for name in ("head pair", "after the loop"):
        plan = ops.gemm_group_plan(SETS[name], 0, 0)
        assert all(p.splits == 1 and not p.fallback for p in plan)
        check_plan(ops, SETS[name], plan, 0, 0)
        plan = ops.gemm_group_plan(SETS[name], 1 << 20, 8)   # tight: whatever splits it picks must fit
        check_plan(ops, SETS[name], plan, 1 << 20, 8)
