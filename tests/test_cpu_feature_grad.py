"""The decoder's gradient with respect to the image features, without a GPU.

* the library exports the three feature-gradient entries and sizes their workspace;
* the decomposition the HIP kernels implement (include/sat_hip.h, sat_decoder_backward_features),

      dL/da = G_ctx + G_W + G_mean / L
      G_ctx[b,l,:] = sum_t alpha[b,t,l] dL/dcontext_t[b,:]                    (attention.py:19-20)
      G_W          = dL/dWs . attention.W.weight                              (attention.py:16)
      G_mean[b,:]  = dL/d[init_h | init_c pre-activations] . [init_h.weight; init_c.weight]   (decoder.py:137-147)

  and without attention (decoder.py:101-105) G_mean += sum_t (d gates_t . W_ih[:, E:] + d f_z,t . f_z.weight),
  restated in torch on this test's own fp64 forward, equals autograd's ``feats.grad`` of the oracle
  (oracle.sat_oracle.decoder_forward + caption_loss, the reference's loss.backward()) to 1e-10.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import sat_oracle as O


def _dims(L, **kw):
    d = L.SatDecoderDims()
    d.B, d.L, d.D, d.E, d.V, d.T = 4, 49, 2048, 512, 1000, 8
    d.tf, d.ado, d.attention, d.dtype = 1, 1, 1, L.SAT_BF16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_library_exports_feature_grad_entries():
    import sat_amd
    L = sat_amd._lib
    lib = L.lib()
    for name in ("sat_decoder_feature_grad_workspace_bytes", "sat_decoder_backward_features",
                 "sat_feature_grad_accumulate"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTED


def test_feature_grad_workspace_bytes():
    import sat_amd
    L = sat_amd._lib
    fn = L.lib().sat_decoder_feature_grad_workspace_bytes
    d8 = _dims(L)
    n8 = fn(ctypes.byref(d8))
    # every step's dL/dcontext [B (T-1), D] fp32 at least
    assert n8 >= 4 * 7 * 2048 * 4
    n16 = fn(ctypes.byref(_dims(L, T=16)))
    assert n16 > n8
    assert n16 - n8 >= 4 * 8 * 2048 * 4
    assert fn(ctypes.byref(_dims(L, T=2))) == 0
    assert fn(ctypes.byref(_dims(L, T=3))) > 0
    assert fn(ctypes.byref(_dims(L, D=2044))) == 0          # D % 8
    assert fn(ctypes.byref(_dims(L, attention=0))) > 0
    # the decoder's own workspace does not depend on it
    assert L.lib().sat_decoder_workspace_bytes(ctypes.byref(d8)) > 0


# ---- the decomposition, on a forward written here (fp64, teacher forcing, no dropout) ----

def _lin(x, p, name):
    return x @ p[name + ".weight"].T + p[name + ".bias"]


def _restated_feature_grad(p, feats, caps, ado, attention):
    """G_ctx + G_W + G_mean / L from quantities the backward kernels hold: alpha, dL/dcontext_t, dL/dWs,
    dL/d(init pre-activations), d gates_t, d f_z,t -- each taken as the autograd gradient of a detached
    intermediate, so nothing here differentiates through the features themselves."""
    B, L, D = feats.shape
    E = p["init_h.weight"].shape[0]
    T1 = caps.shape[1] - 1
    a = feats.detach()

    def leaf(x):
        return x.detach().requires_grad_(True)

    mean = a.mean(1)
    pre0 = leaf(torch.cat((_lin(mean, p, "init_h"), _lin(mean, p, "init_c")), 1))   # [B, 2E]
    h, c = torch.tanh(pre0[:, :E]), torch.tanh(pre0[:, E:])
    Ws = leaf(_lin(a, p, "attention.W")) if attention else None
    ctxs, gates, fz_pre, alphas, preds = [], [], [], [], []
    for t in range(T1):
        emb = p["embedding.weight"][caps[:, t]]
        if attention:
            att = torch.tanh(Ws + _lin(h, p, "attention.U").unsqueeze(1))
            alpha = torch.softmax(_lin(att, p, "attention.v").squeeze(2), 1)
            ctx = (a * alpha.unsqueeze(2)).sum(1)       # a is a constant here: only alpha carries a graph
            ctx.retain_grad()                            # dL/dcontext_t: the gate path + the ado head's f_z path
            ctxs.append(ctx)
            gated = torch.sigmoid(_lin(h, p, "f_beta")) * ctx
        else:
            alpha = torch.full((B, L), 1.0 / L, dtype=a.dtype)
            ctx = gated = mean
        x = torch.cat((emb, gated), 1)
        g = x @ p["lstm.weight_ih"].T + p["lstm.bias_ih"] + h @ p["lstm.weight_hh"].T + p["lstm.bias_hh"]
        g.retain_grad()                                  # d gates_t
        gates.append(g)
        i, f, gg, o = g.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        if ado:
            zp = _lin(ctx, p, "f_z")                     # its gradient: d f_z,t (pre-activation)
            if zp.requires_grad:
                zp.retain_grad()
            else:                                        # a constant of the features alone without attention
                zp = leaf(zp)
            fz_pre.append(zp)
            out = torch.relu(_lin(torch.relu(_lin(h, p, "f_h")) + torch.relu(zp) + emb, p, "f_out"))
        else:
            out = _lin(h, p, "deep_output")
        alphas.append(alpha); preds.append(out)
    preds, alphas_t = torch.stack(preds, 1), torch.stack(alphas, 1)
    O.caption_loss(preds, alphas_t, caps).backward()

    G_mean = pre0.grad @ torch.cat((p["init_h.weight"], p["init_c.weight"]), 0)          # [B, D]
    if attention:
        dctx = torch.stack([x.grad for x in ctxs], 1)                                     # [B, T1, D]
        G_ctx = torch.einsum("btl,btd->bld", alphas_t.detach(), dctx)
        G_W = Ws.grad @ p["attention.W.weight"]                                           # [B, L, D]
        return G_ctx + G_W + (G_mean / L).unsqueeze(1)
    for t in range(T1):
        G_mean = G_mean + gates[t].grad @ p["lstm.weight_ih"][:, -D:]
        if ado:
            G_mean = G_mean + fz_pre[t].grad @ p["f_z.weight"]
    return (G_mean / L).unsqueeze(1).expand(B, L, D)


@pytest.mark.parametrize("attention", [True, False], ids=["att_ado_tf", "noatt_ado_tf"])
def test_decomposition_equals_autograd(attention):
    B, L, D, V, T, E = 3, 16, 64, 60, 9, 512
    p = {k: v.double() for k, v in O.make_decoder_params(V, D, E, True, 21).items()}
    rng = np.random.default_rng(22)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, L, D)), 0)).double()
    caps = O.make_captions(B, T, V, 23)
    a = feats.clone().requires_grad_(True)
    preds, alphas, _ = O.decoder_forward(p, a, caps, tf=True, ado=True, attention=attention)
    O.caption_loss(preds, alphas, caps).backward()
    ref = a.grad
    got = _restated_feature_grad(p, feats, caps, True, attention)
    assert ref.abs().max() > 0
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"decomposition vs autograd ({'att' if attention else 'noatt'}): {err:.3e}")
    assert err < 1e-10
