"""Every GEMM and conv kernel against the one right bit pattern on integer-valued operands (tests/exact_cases.py):
torch.equal with the fp64 reference, rounded to nearest-even once where the output is bf16 -- no tolerance.  bf16
outputs run in both regimes (small: any dropped or added product changes an output; rounding: exact ties, and sums
above 256 quanta under a residual).  tests/test_cpu_exact_cases.py shows on the CPU that each case would notice a
dropped product, a wrong rounding mode and a rounding before the residual add.  Which kernel each case launched is on
record in profiles/exact_integer/kernels.txt.  Every test here needs an MI355X.
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


def dev(t):
    return None if t is None else t.to(DEV)


def same(got, want, what):
    """torch.equal, and on failure how many elements differ, where, and the values."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want) | (torch.isnan(got) != torch.isnan(want))
    idx = bad.nonzero()[:8].tolist()
    vals = [(tuple(i), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx]
    pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first (index, got, want): {vals}")


def cases(*families):
    cs = [c for c in X.CASES if c.family in families]
    return pytest.mark.parametrize("case", cs, ids=[c.id for c in cs])


def run_gemm(sat, case, b):
    from sat_amd import ops
    p, a = dict(case.p), b.args
    M, N = p["M"], p["N"]
    C = dev(a["C0"]) if a["C0"] is not None else torch.full((M, N), float("nan"), dtype=p["cdt"], device=DEV)
    aux = torch.full((M, N), float("nan"), dtype=p["aux"], device=DEV) if p.get("aux") is not None else None
    ops.gemm(dev(a["A"]), dev(a["B"]), C, transA=p["tA"], transB=p["tB"], beta=p.get("beta", 0.0), bias=dev(a["bias"]),
             add1=dev(a["add1"]), act=sat._lib.ACT_RELU if p.get("relu") else sat._lib.ACT_NONE, aux=aux,
             policy=sat.Policy(**dict(case.pol)) if case.pol else None)
    torch.cuda.synchronize()
    same(C, b.outs["C"], f"{case.id} C")
    if aux is not None:
        same(aux, b.outs["aux"], f"{case.id} aux")


def run_conv(sat, case, b):
    from sat_amd import ops
    p, a = dict(case.p), b.args
    y = ops.conv2d_nhwc(dev(a["x"]), dev(a["w"]), dev(a["bias"]), p.get("stride", 1), p.get("pad", 0),
                        bool(p.get("relu")), residual=dev(a["res"]), out_hw=p.get("out_hw"),
                        policy=sat.Policy(**dict(case.pol)) if case.pol else None)
    torch.cuda.synchronize()
    same(y, b.outs["y"], case.id)


@cases("gemm", "split", "skinny")
def test_gemm_kernels(sat, case):
    """gemm_kernel (fp32 operands, as a GEMM and as a conv; bf16 ones the LDS-DMA kernel refuses), split_gemm_kernel,
    skinny_gemm_kernel."""
    (run_gemm if dict(case.p)["kind"] == "gemm" else run_conv)(sat, case, X.build(case))


@cases("fast", "pipe")
def test_tile_kernels(sat, case):
    """fast_gemm_kernel and conv_pipe_kernel, as GEMMs and as convs, in every forced configuration."""
    b = X.build(case)
    (run_gemm if dict(case.p)["kind"] == "gemm" else run_conv)(sat, case, b)


@cases("stream", "ws")
def test_weight_stationary_convs(sat, case):
    """conv1x1_stream_kernel (forced: these problems are below its automatic threshold) and conv_ws_kernel."""
    run_conv(sat, case, X.build(case))


@cases("chain", "proj")
def test_chain_and_proj(sat, case):
    from sat_amd import ops
    b = X.build(case)
    p, a = dict(case.p), b.args
    pol = sat.Policy(**dict(case.pol))
    M, N2 = p["B"] * p["H"] * p["W"], p.get("N2", 0)
    c3 = (dev(a["w"]), dev(a["bias"]), 1, 0)
    c1n = (dev(a["w1"]), dev(a["b1"]), 1, 0) if N2 else None
    if case.family == "proj":
        assert ops.conv1x1_proj_supported(M, p["K"], p["N"], p["Kp"], p["S"], N2, X.BF, pol)
        res = ops.ProjectedResidual(dev(a["xin"]), (dev(a["wp"]), dev(a["bp"]), p["S"], 0))
    else:
        assert ops.conv1x1_chain_supported(M, p["K"], p["N"], N2, X.BF, pol)
        res = dev(a["res"])
    if N2:
        y, x1 = ops.conv1x1_chain(dev(a["x"]), c3, res, c1n, policy=pol)
    else:
        y, x1 = ops.conv2d_nhwc(dev(a["x"]), *c3, True, residual=res, policy=pol), None
    torch.cuda.synchronize()
    same(y, b.outs["y"], f"{case.id} y")
    if N2:
        same(x1, b.outs["x1"], f"{case.id} x1")


@cases("stempool")
def test_stem_pool(sat, case):
    from sat_amd import ops
    b = X.build(case)
    p, a = dict(case.p), b.args
    x, w = dev(a["x"]), dev(a["w"])
    assert ops.conv_stem_pool_supported(x, w, 1, p["pad"], True, p["pool"], p["out_hw"])
    y = ops.conv_stem_pool(x, w, dev(a["bias"]), 1, p["pad"], True, p["pool"], out_hw=p["out_hw"])
    torch.cuda.synchronize()
    same(y, b.outs["y"], case.id)


@cases("pool")
def test_maxpool(sat, case):
    from sat_amd import ops
    b = X.build(case)
    y = ops.maxpool2d_nhwc(dev(b.args["x"]), *dict(case.p)["pool"])
    torch.cuda.synchronize()
    same(y, b.outs["y"], case.id)


@cases("frag3x3", "frag1x1")
def test_fragment_convs(sat, case):
    """convblock.hip's register-direct 3x3 and 1x1 kernels at every geometry they accept: three images and the first
    alone, every conv_slices form the geometry has."""
    from sat_amd import ops
    b = X.build(case)
    p, a = dict(case.p), b.args
    H, C, Cout = p["H"], p["C"], p["Cout"]
    x, w, bias = dev(a["x"]), dev(a["w"]), dev(a["bias"])
    f = (ops.mfma_frag_layout(w.reshape(Cout, -1)), bias)
    if case.family == "frag3x3":
        assert ops.conv3x3_frag_supported(H, H, C, X.BF)
        forms = (0, 1, 2) if (H, C) in ((14, 256), (7, 512)) else (0,)
    else:
        assert ops.conv1x1_frag_supported(H, H, C, Cout, X.BF)
        forms = (0, 1, 2)
    call = ops.conv3x3_frag if case.family == "frag3x3" else ops.conv1x1_frag
    for n in (3, 1):
        for s in forms:
            y = call(x[:n].contiguous(), f, policy=sat.Policy(conv_slices=s))
            torch.cuda.synchronize()
            same(y, b.outs["y"][:n], f"{case.id} N={n} conv_slices={s}")


@cases("block")
def test_bottleneck_fused(sat, case):
    from sat_amd import ops
    b = X.build(case)
    p, a = dict(case.p), b.args
    assert ops.bottleneck_fused_supported(p["H"], p["H"], p["C"], p["Cmid"], X.BF)
    x = dev(a["x"])
    frags = [(ops.mfma_frag_layout(dev(a[w]).reshape(a[w].shape[0], -1)), dev(a[bn]))
             for w, bn in (("w1", "b1"), ("w2", "b2"), ("w3", "b3"))]
    for n in (3, 1):
        y = ops.bottleneck_fused(x[:n].contiguous(), *frags)
        torch.cuda.synchronize()
        same(y, b.outs["y"][:n], f"{case.id} N={n}")


@cases("wgrad")
def test_conv3x3_wgrad(sat, case):
    """bf16 (the split-K kernel, with a workspace and unsplit without) and fp32 (im2col + the fp32 GEMM)."""
    from sat_amd import ops
    b = X.build(case)
    p, a = dict(case.p), b.args
    x, dz = dev(a["x"]), dev(a["dz"])
    assert ops.conv3x3_wgrad_workspace_bytes(x.shape, p["Cout"], p["dtype"]) > 0
    for ws in ((True, None) if p["dtype"] == X.BF else (True,)):
        out = dev(a["prior"]).clone() if p["accumulate"] else torch.full((p["Cout"], 3, 3, p["Cin"]), float("nan"),
                                                                         device=DEV)
        ops.conv3x3_wgrad(x, dz, out=out, accumulate=p["accumulate"], workspace=ws)
        torch.cuda.synchronize()
        same(out, b.outs["dw"], f"{case.id} workspace={ws}")
