"""split_gemm_group_kernel (csrc/gemmsplit.hip): independent products of the deterministic split-K GEMM as one launch,
through sat_gemm_group (n products, each with its own policy).

Before every run the workspace (partial tiles and tickets) and every beta = 0 output are filled with NaN bit patterns;
a beta = 1 output and an fp32 addend are inputs and are rebuilt instead.  The call zeroes its tickets with one zeroing
launch on the stream before the group, as the decoder backward does per phase.

(a) a three-product group with forced plans equals three sat_gemm calls with the same plans bit for bit, and a group
    of one equals sat_gemm; (b) on the integer-valued operands of tests/exact_cases.py the same group equals the exact
    products; (c) so does a group with more blocks than CUs (a 320-tile product first, then a split one: blocks past
    the first round, slab and ticket indexing past the first product); (d) two runs from poisoned buffers give the
    same bits; (e) the decoder backward.  The smallest attention + ado bf16 decoder of tests/test_gpu_shapes.py has
    28 rows B (T - 1), below the 2560 from which the backward groups, so it issues one launch per product under every
    policy: it meets that test's gradient bound under the default policy, with every product forced onto the split
    kernel and with split_gemm = 4, and its captured backward replays bit-identically.  The groups themselves run at
    bench.py's B = 128 instance (3328 rows; sat_gemm_group_launches counts them): its grouped backward equals the
    ungrouped one bit for bit, and, captured into a graph and replayed twice over NaN-poisoned gradients, gives
    finite and identical bits -- each phase's zeroing launch covers its group's tickets on every replay.
"""
import pytest
import torch

import exact_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


# name: M, N, K, transA, transB, beta, fp32 addend, (split_gemm, split_k)
P1 = ("P1", 264, 136, 328, True, True, 0.0, False, (2, 2))    # 3 x 2 tiles with row / column edges, K tail of 8
P2 = ("P2", 128, 128, 64, False, True, 0.0, False, (2, 1))    # B k-major only, one k-tile
P3 = ("P3", 8, 8, 8, True, True, 1.0, True, (2, 1))           # beta = 1 over a prefilled C, fp32 addend
BIG = ("BIG", 2560, 2048, 128, True, True, 0.0, False, (2, 1))   # 20 x 16 = 320 tiles of 128 rows: two rounds


def _random(spec, seed):
    name, M, N, K, tA, tB, beta, add1, _ = spec
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).bfloat16()
    Bm = torch.randn(N, K, generator=g).bfloat16()
    return dict(A=(A.T.contiguous() if tA else A), B=(Bm.T.contiguous() if tB else Bm),
                C0=torch.randn(M, N, generator=g) if beta else None,
                add1=torch.randn(M, N, generator=g) if add1 else None)


def _exact(spec):
    name, M, N, K, tA, tB, beta, add1, _ = spec
    case = X.Case(f"group-{name}", "split", "small",
                  X._p("gemm", M=M, N=N, K=K, tA=tA, tB=tB, dtype=X.BF, cdt=X.F32, beta=beta,
                       add1=X.F32 if add1 else None), ())
    b = X.build(case)
    return dict(A=b.args["A"], B=b.args["B"], C0=b.args["C0"], add1=b.args["add1"]), b.outs["C"]


def _product(sat, spec, data, policy=True):
    """gemm keywords of one product on fresh device buffers: C a view inside a NaN-filled buffer (beta = 1: prefilled)."""
    name, M, N, K, tA, tB, beta, add1, form = spec
    big = torch.full((M + 3, N + 8), float("nan"), device=DEV)
    C = big[:M, :N]
    if beta:
        C.copy_(data["C0"].to(DEV))
    kw = dict(A=data["A"].to(DEV), B=data["B"].to(DEV), C=C, transA=tA, transB=tB, beta=beta,
              add1=data["add1"].to(DEV) if add1 else None)
    if policy:
        kw["policy"] = sat.Policy(split_gemm=form[0], split_k=form[1])
    return kw, big


def _workspace(sat):
    n = int(sat._lib.lib().sat_gemm_group_workspace_bytes())
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)   # NaN words: partial tiles and tickets


def _run_group(sat, specs, datas, policy=True):
    from sat_amd import ops
    prods = [_product(sat, s, d, policy) for s, d in zip(specs, datas)]
    ops.gemm_group([kw for kw, _ in prods], _workspace(sat))
    torch.cuda.synchronize()
    outs = []
    for (kw, big), s in zip(prods, specs):
        M, N = s[1], s[2]
        assert torch.isnan(big[M:]).all() and torch.isnan(big[:, N:]).all(), s[0]   # nothing outside C
        assert torch.isfinite(kw["C"]).all(), s[0]
        outs.append(kw["C"].clone())
    return outs


def _run_single(sat, spec, data, policy=True):
    from sat_amd import ops
    kw, _ = _product(sat, spec, data, policy)
    ws = torch.full((int(sat._lib.lib().sat_gemm_workspace_bytes()),), 0xFF, dtype=torch.uint8, device=DEV)
    C = kw.pop("C")
    ops.gemm(kw.pop("A"), kw.pop("B"), C, workspace=ws, **kw)
    torch.cuda.synchronize()
    return C.clone()


@pytest.fixture(scope="module")
def random_data():
    return [_random(s, 17 + i) for i, s in enumerate((P1, P2, P3))]


def test_group_equals_single_launches_bit_for_bit(sat, random_data):
    """(a) Same plan, same bits: the group runs the single launch's body on each (tile, split)."""
    specs = (P1, P2, P3)
    grouped = _run_group(sat, specs, random_data)
    for s, d, g in zip(specs, random_data, grouped):
        single = _run_single(sat, s, d)
        assert torch.equal(g, single), s[0]
        A = d["A"].double().T if s[4] else d["A"].double()
        Bm = d["B"].double().T if s[5] else d["B"].double()
        ref = A @ Bm.T + (d["add1"].double() if s[7] else 0) + (d["C0"].double() if s[6] else 0)
        err = ((g.double().cpu() - ref).norm() / ref.norm()).item()
        assert err < 2e-5, (s[0], err)   # fp32 accumulation of exact bf16 products (tests/test_gpu_gemm_split.py)


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_group_of_one_equals_sat_gemm(sat, random_data, idx):
    """(a) A group of one product is that product's own launch: sat_gemm's bits."""
    spec = (P1, P2, P3)[idx]
    g = _run_group(sat, (spec,), (random_data[idx],))[0]
    assert torch.equal(g, _run_single(sat, spec, random_data[idx])), spec[0]


def test_group_exact_on_integer_inputs(sat):
    """(b) Integer-valued operands: one right bit pattern whatever the tile height, split count and sum order."""
    specs = (P1, P2, P3)
    built = [_exact(s) for s in specs]
    for rows in (2, 3):   # 128-row and 256-row tiles
        forced = [s[:8] + ((rows, s[8][1]),) for s in specs]
        outs = _run_group(sat, forced, [d for d, _ in built])
        for s, o, (_, ref) in zip(specs, outs, built):
            assert torch.equal(o.cpu(), ref), (s[0], rows)


def test_group_with_more_blocks_than_cus(sat):
    """(c) 320 unsplit tiles beside the split P1: 332 blocks, so blocks of a second round and a product whose blocks
    start past another's; then with a second split product, whose slab region and tickets lie behind P1's."""
    from sat_amd import ops
    plan = ops.gemm_group_plan([(2560, 2048, 128, 128, 1), (264, 136, 328, 128, 2)], 1 << 25, 1024)
    assert sum(p.blocks for p in plan) == 332 and sorted(p.first_block for p in plan) in ([0, 12], [0, 320])
    P1B = ("P1B",) + P1[1:8] + ((3, 2),)
    for specs in ((BIG, P1), (P1, BIG, P1B)):
        built = [_exact(s) for s in specs]
        outs = _run_group(sat, specs, [d for d, _ in built])
        for s, o, (_, ref) in zip(specs, outs, built):
            assert torch.equal(o.cpu(), ref), s[0]


def test_group_bit_identical_across_runs(sat, random_data):
    """(d) Split order, not arrival order: two runs from poisoned buffers agree bit for bit."""
    specs = (P1, P2, P3)
    a = _run_group(sat, specs, random_data)
    b = _run_group(sat, specs, random_data)
    for s, x, y in zip(specs, a, b):
        assert torch.equal(x, y), s[0]


@pytest.mark.parametrize("splits", [1, 2, 3])
def test_tile_height_does_not_change_the_bits(sat, splits):
    """What lets the decoder's groups choose tile heights freely while every member keeps its single launch's split
    count: at one split count, 128-row and 256-row tiles add each output element's k-tiles in the same order."""
    from sat_amd import ops
    for seed, (M, N, K, tA, tB) in enumerate([(264, 136, 712, True, True), (300, 136, 520, False, True)]):
        g = torch.Generator().manual_seed(40 + seed)
        A = torch.randn(M, K, generator=g).bfloat16()
        Bm = torch.randn(N, K, generator=g).bfloat16()
        Ad, Bd = (A.T.contiguous() if tA else A).to(DEV), (Bm.T.contiguous() if tB else Bm).to(DEV)
        outs = []
        for rows in (2, 3):
            C = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(Ad, Bd, C, transA=tA, transB=tB, policy=sat.Policy(split_gemm=rows, split_k=splits))
            outs.append(C)
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]), (M, N, K, splits)


# ---------------------------------------------------------------------------- (e) the decoder backward
GROUPS_PER_BACKWARD = 2   # the head's four products, the products after the time loop (csrc/decoder.hip)


def _launches(sat):
    return int(sat._lib.lib().sat_gemm_group_launches())


def test_bench_instance_gradients_equal_the_single_launches_bit_for_bit(sat):
    """bench.py's B = 128 decoder instance: the grouped backward (the default) and the backward with every product
    launched on its own (SatPolicy.split_gemm = 4) give the same gradients and updated parameters, bit for bit --
    every member of a group keeps its single launch's split count."""
    import test_gpu_shapes as S
    c = S._bench_case("b128_tf_st96")
    n0 = _launches(sat)
    a = S._hip_step(sat, c, torch.bfloat16, split_target=c["split_target"])
    n1 = _launches(sat)
    b = S._hip_step(sat, c, torch.bfloat16, split_target=c["split_target"], policy=sat.Policy(split_gemm=4))
    assert (n1 - n0, _launches(sat) - n1) == (GROUPS_PER_BACKWARD, 0)
    assert a["loss"] == b["loss"] and torch.equal(a["preds"], b["preds"]) and torch.equal(a["alphas"], b["alphas"])
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n
        assert torch.equal(a["params"][n], b["params"][n]), n


@pytest.fixture(scope="module")
def shapes():
    import test_gpu_shapes as S
    c = S._case("resnet_ado_tf")
    return S, c, S._oracle(c, torch.float32)


@pytest.mark.parametrize("split_gemm", [0, 2, 4], ids=["default", "split-kernel-forced", "split_gemm-4"])
def test_small_decoder_gradients_meet_the_existing_bound(sat, shapes, split_gemm):
    """The bound and the check are tests/test_gpu_shapes.py's own (test_production_shape_bf16_close_to_oracle).  28
    rows: no groups under any policy; split_gemm = 2 also sends the K = 28 weight gradients to the split kernel."""
    S, c, o32 = shapes
    n0 = _launches(sat)
    h = S._hip_step(sat, c, torch.bfloat16, policy=sat.Policy(split_gemm=split_gemm) if split_gemm else None)
    assert _launches(sat) == n0
    S._assert_bf16(c, h, o32, grad_tol=S.SHAPES_BF16_GRAD_TOL)


@pytest.mark.parametrize("case", ["small", "bench-b128"])
def test_decoder_backward_replays_bit_identically(sat, shapes, case):
    """A captured forward + backward, replayed twice over NaN-poisoned gradients: finite, and the same bits.  At the
    bench instance the capture must hold the two grouped launches, whose tickets only the phases' zeroing launches
    reset between replays."""
    S = shapes[0]
    c, groups = (shapes[1], 0) if case == "small" else (S._bench_case("b128_tf_st96"), GROUPS_PER_BACKWARD)
    dec = S._decoder(sat, c).eval()
    dec.split_target = c.get("split_target", 0)
    opt = sat.Adam(dec.parameters(), lr=S.LR)
    caps, feats = c["caps"].to(DEV), c["feats"].to(DEV).bfloat16()

    def step():
        preds, alphas = dec(feats, caps)
        sat.caption_loss(preds, alphas, caps)[0].backward()
    opt.zero_grad(set_to_none=True)
    step()   # eager warm-up (allocations), then the capture
    torch.cuda.synchronize()
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    n0 = _launches(sat)
    with torch.cuda.graph(graph):
        step()
    assert _launches(sat) - n0 == groups
    params = dict(dec.named_parameters())
    active = [(n, dec._offsets[n], params[n].numel()) for n in dec.active_param_names()]
    runs = []
    for _ in range(2):
        dec._grad_flat.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        runs.append(dec._grad_flat.clone())
    assert _launches(sat) - n0 == groups   # a replay issues nothing from the host
    for n, o, m in active:
        assert torch.isfinite(runs[0][o:o + m]).all(), n
        assert torch.equal(runs[0][o:o + m], runs[1][o:o + m]), n
