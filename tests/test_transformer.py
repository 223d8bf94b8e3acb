"""SeqFormer deformable transformer (callers of rows a4) against a fixture produced
by the reference's own deformable_transformer.py (oracle/make_golden_transformer.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle import msda_oracle as O
from vnext_amd.models.seqformer_transformer import DeformableTransformer
from vnext_amd.ops.functions import ms_deform_attn_func as func_mod


def load():
    return dict(np.load(os.path.join(GOLDEN_DIR, "transformer_seqformer.npz")))


def build(g, device, dtype):
    C, M, L, P, T, ne, nd, ff = (int(x) for x in g["cfg"])
    tr = DeformableTransformer(d_model=C, nhead=M, num_encoder_layers=ne, num_decoder_layers=nd,
                               dim_feedforward=ff, dropout=0.0, return_intermediate_dec=True, num_frames=T,
                               num_feature_levels=L, dec_n_points=P, enc_n_points=P)
    tr.decoder.bbox_embed = torch.nn.ModuleList(
        [torch.nn.Sequential(torch.nn.Linear(C, C), torch.nn.ReLU(), torch.nn.Linear(C, 4)) for _ in range(nd)])
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}
    assert set(sd) == set(tr.state_dict()), "state-dict keys must match the reference transformer"
    tr = tr.to(torch.float64)
    tr.load_state_dict(sd)
    return tr.to(device=device, dtype=dtype).eval(), L


def run(tr, L, g, device, dtype):
    srcs = [torch.from_numpy(g[f"src{i}"]).to(device, dtype) for i in range(L)]
    poss = [torch.from_numpy(g[f"pos{i}"]).to(device, dtype) for i in range(L)]
    masks = [torch.from_numpy(g[f"mask{i}"]).to(device) for i in range(L)]
    with torch.no_grad():
        return tr(srcs, masks, poss, torch.from_numpy(g["query_embed"]).to(device, dtype))


class _OracleOp:
    @staticmethod
    def ms_deform_attn_forward(value, shapes, lsi, loc, attn, im2col_step):
        return torch.from_numpy(O.msda_forward(value.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), attn.numpy()))


def check(out, g, tol):
    hs, hs_box, memory, init_ref, inter_refs, _, _, valid_ratios = out
    for name, t in (("hs", hs), ("hs_box", hs_box), ("memory", memory), ("init_ref", init_ref),
                    ("inter_refs", inter_refs), ("valid_ratios", valid_ratios)):
        assert tuple(t.shape) == g[name].shape, name
        np.testing.assert_allclose(t.double().cpu().numpy(), g[name], rtol=0,
                                   atol=tol * max(1.0, float(np.abs(g[name]).max())), err_msg=name)


def test_transformer_host_logic_matches_reference_cpu(monkeypatch):
    monkeypatch.setattr(func_mod, "MSDA", _OracleOp)
    g = load()
    tr, L = build(g, "cpu", torch.float64)
    check(run(tr, L, g, "cpu", torch.float64), g, 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-8), (torch.float32, 2e-4)])
def test_transformer_on_gpu(dtype, tol):
    g = load()
    tr, L = build(g, "cuda:0", dtype)
    check(run(tr, L, g, "cuda:0", dtype), g, tol)


# ---------------------------------------------------------------- IDOL (per-frame) transformer
def load_idol():
    return dict(np.load(os.path.join(GOLDEN_DIR, "transformer_idol.npz")))


def build_idol(g, device, dtype):
    from vnext_amd.models.idol_transformer import DeformableTransformer as IdolTransformer
    C, M, L, P, ne, nd, ff = (int(x) for x in g["cfg"])
    tr = IdolTransformer(d_model=C, nhead=M, num_encoder_layers=ne, num_decoder_layers=nd, dim_feedforward=ff,
                         dropout=0.0, return_intermediate_dec=True, num_feature_levels=L, dec_n_points=P,
                         enc_n_points=P, return_samples=True)
    tr.decoder.bbox_embed = torch.nn.ModuleList(
        [torch.nn.Sequential(torch.nn.Linear(C, C), torch.nn.ReLU(), torch.nn.Linear(C, 4)) for _ in range(nd)])
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}
    assert set(sd) == set(tr.state_dict()), "state-dict keys must match the reference transformer"
    tr = tr.to(torch.float64)
    tr.load_state_dict(sd)
    return tr.to(device=device, dtype=dtype).eval(), L


def check_idol(out, g, tol):
    hs, memory, init_ref, inter_refs, inter_samples, _, _ = out
    for name, t in (("hs", hs), ("memory", memory), ("init_ref", init_ref), ("inter_refs", inter_refs),
                    ("inter_samples", inter_samples)):
        assert tuple(t.shape) == g[name].shape, name
        np.testing.assert_allclose(t.double().cpu().numpy(), g[name], rtol=0,
                                   atol=tol * max(1.0, float(np.abs(g[name]).max())), err_msg=name)


def test_idol_transformer_host_logic_matches_reference_cpu(monkeypatch):
    monkeypatch.setattr(func_mod, "MSDA", _OracleOp)
    g = load_idol()
    tr, L = build_idol(g, "cpu", torch.float64)
    check_idol(run(tr, L, g, "cpu", torch.float64), g, 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-8), (torch.float32, 2e-4)])
def test_idol_transformer_on_gpu(dtype, tol):
    g = load_idol()
    tr, L = build_idol(g, "cuda:0", dtype)
    out = run(tr, L, g, "cuda:0", dtype)
    if dtype == torch.float32:   # the top-30 order of near-equal weights may differ in fp32
        out = out[:4] + (torch.from_numpy(g["inter_samples"]),) + out[5:]
    check_idol(out, g, tol)


# ---------------------------------------------------------------- state-dict key ORDER (what seeded initialisation walks)
def _wb(*names):
    return [f"{n}.{p}" for n in names for p in ("weight", "bias")]


_MHA = ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
_MSDA = ["sampling_offsets", "attention_weights", "value_proj", "output_proj"]      # the module's Linears, construction order


def _expected_keys(encoder_layer, decoder_layer, layers=2):
    keys = ["level_embed"]
    for stack, layer in (("encoder", encoder_layer), ("decoder", decoder_layer)):
        keys += [f"{stack}.layers.{i}.{k}" for i in range(layers) for k in layer]
    return keys + _wb("reference_points")


@pytest.mark.parametrize("kind", ["seqformer", "idol"])
def test_state_dict_key_order(kind):
    """Per layer: the attention module's Linears in construction order, then the norms and Linears in registration order.
    `_reset_parameters` walks the parameters in this order, so it is part of what a seed means."""
    from vnext_amd.models.idol_transformer import DeformableTransformer as IdolTransformer
    if kind == "seqformer":
        cls, msda = DeformableTransformer, _MSDA + ["output_proj_box"]
        decoder_layer = (_wb(*(f"cross_attn.{n}" for n in msda)) + _wb("norm1", "norm1_box")
                         + [f"self_attn.{k}" for k in _MHA] + _wb("norm2") + [f"self_attn_box.{k}" for k in _MHA]
                         + _wb("norm2_box", "linear1", "linear2", "norm3", "linear1_box", "linear2_box", "norm3_box",
                               "time_attention_weights"))
    else:
        cls, msda = IdolTransformer, _MSDA
        decoder_layer = (_wb(*(f"cross_attn.{n}" for n in msda)) + _wb("norm1") + [f"self_attn.{k}" for k in _MHA]
                         + _wb("norm2", "linear1", "linear2", "norm3"))
    encoder_layer = _wb(*(f"self_attn.{n}" for n in msda)) + _wb("norm1", "linear1", "linear2", "norm2")
    tr = cls(d_model=64, nhead=2, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=128,
             return_intermediate_dec=True, num_feature_levels=4)
    want = _expected_keys(encoder_layer, decoder_layer)
    assert len(want) == {"seqformer": 119, "idol": 79}[kind]
    assert list(tr.state_dict()) == want


# ---------------------------------------------------------------- gradients against the reference (train() mode)
def _fixture_gradients(kind, g, gg, tr, L):
    """fp64 on the CPU, MSDA through F.grid_sample: the fixture's upstream gradients on what the detector consumes, then every
    gradient (each parameter, src{i}, pos{i}, query_embed) and the box predictions within 1e-9 of the reference's.  The set of
    tensors that receive a gradient must be the reference's: that pins what is detached where.  (The 1e-12 floor is for
    time_attention_weights.bias, whose gradient is zero in exact arithmetic -- the softmax over the frames does not see a
    shift -- and ~1e-15 of rounding on both sides; every other gradient here is above 0.2.)"""
    import model_grad_harness as H
    tr.train()
    srcs = [torch.from_numpy(g[f"src{i}"]).requires_grad_(True) for i in range(L)]
    poss = [torch.from_numpy(g[f"pos{i}"]).requires_grad_(True) for i in range(L)]
    masks = [torch.from_numpy(g[f"mask{i}"]) for i in range(L)]
    query_embed = torch.from_numpy(g["query_embed"]).requires_grad_(True)
    with H.aten_baseline(tr):
        outs = H.outputs(kind, tr, srcs, masks, poss, query_embed)
        assert {k[2:] for k in gg if k.startswith("G.")} == set(outs)
        sum((torch.from_numpy(gg[f"G.{k}"]) * v).sum() for k, v in outs.items()).backward()
    got = {f"grad.{n}": p.grad for n, p in tr.named_parameters() if p.grad is not None}
    for i in range(L):
        got[f"grad.src{i}"], got[f"grad.pos{i}"] = srcs[i].grad, poss[i].grad
    got["grad.query_embed"] = query_embed.grad
    got["boxes"] = outs["boxes"].detach()
    want = {k: v for k, v in gg.items() if not k.startswith("G.")}
    assert set(got) == set(want), f"missing {sorted(set(want) - set(got))}, extra {sorted(set(got) - set(want))}"
    for k in sorted(want):
        assert tuple(got[k].shape) == want[k].shape, k
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=0, atol=1e-9 * float(np.abs(want[k]).max()) + 1e-12,
                                   err_msg=k)


def test_transformer_gradients_match_reference_cpu():
    g = load()
    gg = dict(np.load(os.path.join(GOLDEN_DIR, "transformer_seqformer_grad.npz")))
    tr, L = build(g, "cpu", torch.float64)
    _fixture_gradients("seqformer", g, gg, tr, L)


def test_idol_transformer_gradients_match_reference_cpu():
    g = load_idol()
    gg = dict(np.load(os.path.join(GOLDEN_DIR, "transformer_idol_grad.npz")))
    tr, L = build_idol(g, "cpu", torch.float64)
    tr.decoder.return_samples = False       # the training path: no sample keeper
    _fixture_gradients("idol", g, gg, tr, L)
