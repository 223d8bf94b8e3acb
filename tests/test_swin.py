"""Swin backbone (vnext_amd/models/swin.py) against the reference's backbone/swin.py: tests/golden/swin_*.npz
(tools/make_golden_swin.py, float64), the state-dict names a reference checkpoint carries, the cfg wiring of SeqFormer and
IDOL, and -- on the GPU -- the same fixtures through the fused window-attention kernel and the models' training steps."""
import os

import numpy as np
import pytest
import torch

import swin_golden_recipe as R
from conftest import GOLDEN_DIR
from vnext_amd import _lib
from vnext_amd import train as T
from vnext_amd.models.seqformer import ResNet50Trunk
from vnext_amd.models.swin import D2SwinTransformer, SwinTransformer, SwinTransformerBlock
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg

SMALL_SWIN = {"MODEL.BACKBONE.NAME": "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM": 32, "MODEL.SWIN.DEPTHS": [2, 2, 2, 2],
              "MODEL.SWIN.NUM_HEADS": [1, 2, 4, 8], "MODEL.SWIN.WINDOW_SIZE": 7, "MODEL.SWIN.DROP_PATH_RATE": 0.2}
SEQ_TINY = {"MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 2, "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 12,
            "MODEL.SeqFormer.DIM_FEEDFORWARD": 64, "MODEL.SeqFormer.DROPOUT": 0.0, "INPUT.SAMPLING_FRAME_NUM": 2}
IDOL_TINY = {"MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 2, "MODEL.IDOL.NUM_OBJECT_QUERIES": 110,
             "MODEL.IDOL.DIM_FEEDFORWARD": 64, "MODEL.IDOL.DROPOUT": 0.0}


def _fixture(name):
    return np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))


def _build(name, device, dtype):
    """-> module, input (leaf, requires grad), outputs dict, with the recipe's weights (digest checked)"""
    case = R.CASES[name]
    torch.manual_seed(0)
    if case["kind"] == "model":
        module = SwinTransformer(embed_dim=case["embed_dim"], depths=case["depths"], num_heads=case["num_heads"],
                                 window_size=case["window_size"], drop_path_rate=0.0).double()
    else:
        module = SwinTransformerBlock(case["dim"], case["num_heads"], case["window_size"], case["shift_size"]).double()
    R.fill_params(module, case["seed"])
    x = R.make_input(case)
    assert R.digest(module, x) == str(_fixture(name)["digest"]), f"{name}: regenerated weights / input differ"
    module = module.to(device, dtype)
    x = x.to(device, dtype).requires_grad_(True)
    return module, x


def _forward(name, module, x):
    case = R.CASES[name]
    if case["kind"] == "model":
        return module(x)
    return {"out": module(x, case["H"], case["W"])}


def _max_rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(1e-30, float(np.abs(want).max()))


def _compare(name, device, dtype, tol):
    module, x = _build(name, device, dtype)
    outputs = _forward(name, module, x)
    R.loss(outputs, R.loss_weights({k: v.cpu() for k, v in outputs.items()}, R.CASES[name]["seed"])).backward()
    got = R.summarise({k: v.double().cpu() for k, v in outputs.items()}, x.grad.double().cpu(),
                      dict(module.named_parameters()), R.CASES[name]["seed"])
    want = _fixture(name)
    keys = [k for k in want.files if k not in ("digest", "state_keys")]
    assert sorted(keys) == sorted(got), "fixture / module arrays differ"
    errs = {k: _max_rel(got[k], want[k]) for k in keys}
    bad = {k: e for k, e in errs.items() if not e <= tol}
    assert not bad, bad
    return module, errs


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_torch_expression_matches_reference_fixture(name):
    """CPU (the reference expression, by torch), float64: outputs, input and parameter gradients."""
    _compare(name, "cpu", torch.float64, 1e-9)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_state_dict_names_are_the_reference_checkpoints(name):
    module, _ = _build(name, "cpu", torch.float64)
    assert list(module.state_dict()) == [str(k) for k in _fixture(name)["state_keys"]]


def test_relative_position_index_is_a_buffer_and_not_a_parameter():
    blk = SwinTransformerBlock(64, 2, window_size=7, shift_size=3)
    assert "attn.relative_position_index" in dict(blk.named_buffers())
    assert tuple(blk.attn.relative_position_bias_table.shape) == (169, 2)
    idx = blk.attn.relative_position_index
    assert int(idx.min()) == 0 and int(idx.max()) == 168 and int(idx[0, 0]) == 84


def test_build_model_swin_and_default_backbones():
    swin = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **SEQ_TINY, **SMALL_SWIN}))
    bb = swin.detr.detr.backbone
    assert isinstance(bb, D2SwinTransformer)
    assert bb.num_channels == (64, 128, 256) and bb.strides == (8, 16, 32)
    assert not any(p.requires_grad for p in bb.norm0.parameters())           # res2 is never read (norm0 kept for the checkpoint)
    assert all(p.requires_grad for n, p in bb.named_parameters() if not n.startswith("norm0."))
    # every Swin parameter lands in the backbone's 0.1x group
    opt = T.build_optimizer(swin)
    lrs = {id(p): g["lr"] for g in opt.param_groups for p in g["params"]}
    assert {lrs[id(p)] for p in bb.parameters() if p.requires_grad} == {2e-4 * 0.1}
    idol = build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **IDOL_TINY, **SMALL_SWIN}))
    assert isinstance(idol.detr.detr.backbone, D2SwinTransformer)
    # the default cfg: the ResNet-50 trunk, and not one state-dict key of a Swin
    for model in (build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **SEQ_TINY})),
                  build_model(get_idol_cfg(**{"MODEL.DEVICE": "cpu", **IDOL_TINY}))):
        assert type(model.detr.detr.backbone) is ResNet50Trunk
        assert not any("relative_position" in k for k in model.state_dict())


def test_swin_forward_shapes_and_dict_interface():
    cfg = get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **SMALL_SWIN})
    bb = D2SwinTransformer(cfg).eval()
    x = torch.randn(1, 3, 96, 160)
    with torch.no_grad():
        feats = bb(x)
        d = bb.features(x)
    assert [tuple(f.shape) for f in feats] == [(1, 64, 12, 20), (1, 128, 6, 10), (1, 256, 3, 5)]
    assert sorted(d) == ["res2", "res3", "res4", "res5"]
    for f, k in zip(feats, ("res3", "res4", "res5")):
        torch.testing.assert_close(f, d[k])


def test_drop_path_schedule_and_frozen_stages():
    m = SwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.3, frozen_stages=2)
    rates = [getattr(b.drop_path, "drop_prob", 0.0) for layer in m.layers for b in layer.blocks]
    np.testing.assert_allclose(rates, np.linspace(0, 0.3, 8), rtol=1e-6)
    assert not any(p.requires_grad for p in m.patch_embed.parameters())
    assert not any(p.requires_grad for p in m.layers[0].parameters())
    assert all(p.requires_grad for p in m.layers[1].parameters())
    m.train()
    assert not m.layers[0].training and m.layers[1].training
    with pytest.raises(NotImplementedError):
        SwinTransformer(ape=True)


def test_capture_training_graphs_rejects_swin():
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cpu", **SEQ_TINY, **SMALL_SWIN}))
    with pytest.raises(NotImplementedError):
        T.capture_training_graphs(model, [])


# ---- GPU -----------------------------------------------------------------------------------------------------------------

@pytest.fixture
def forward_counter(monkeypatch):
    """counts the calls of vnx_window_attention_forward made through the package"""
    lib = _lib.lib()
    real = lib.vnx_window_attention_forward
    calls = [0]

    class Counting:
        def __getattr__(self, name):
            return getattr(lib, name)

        def vnx_window_attention_forward(self, *args):
            calls[0] += 1
            return real(*args)
    monkeypatch.setattr(_lib, "lib", lambda: Counting())
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fused_kernel_matches_reference_fixture_on_gpu(name, forward_counter):
    """fp32 on the GPU, the window attention through the HIP kernel: within 2e-3 of the float64 reference (scaled by each
    array's largest element) -- outputs, input gradient and every parameter gradient."""
    _, errs = _compare(name, "cuda:0", torch.float32, 2e-3)
    case = R.CASES[name]
    assert forward_counter[0] == (sum(case["depths"]) if case["kind"] == "model" else 1)
    print(name, "max error", max(errs.values()))


@pytest.mark.gpu
def test_swin_under_bf16_autocast_on_gpu(forward_counter):
    """Under torch.autocast(bfloat16) the GEMMs run in bf16 and the window-attention core in fp32: the outputs are finite and
    within 5e-2 of the fp32 outputs (scaled by each output's largest element)."""
    module, x = _build("swin_w7", "cuda:0", torch.float32)
    with torch.no_grad():
        ref = module(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp = module(x)
    assert forward_counter[0] == 2 * 8
    for k in ref:
        assert torch.isfinite(amp[k]).all()
        assert _max_rel(amp[k].float().cpu().numpy(), ref[k].cpu().numpy()) < 5e-2, k


def _swin_step(arch):
    torch.manual_seed(31)
    if arch == "SeqFormer":
        cfg = get_seqformer_cfg(**{"MODEL.DEVICE": "cuda:0", **SEQ_TINY, **SMALL_SWIN})
    else:
        cfg = get_idol_cfg(**{"MODEL.DEVICE": "cuda:0", **IDOL_TINY, **SMALL_SWIN})
    model = build_model(cfg).train()
    clips = T.synthetic_clips(2, 2, 96, 160, "cuda:0", seed=5, num_instances=2)
    losses = model(clips)
    assert all(torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    bb = model.detr.detr.backbone
    dead = [n for n, p in bb.named_parameters() if p.requires_grad and (p.grad is None or not float(p.grad.abs().sum()) > 0)]
    assert not dead, dead
    assert all(torch.isfinite(p.grad).all() for p in bb.parameters() if p.grad is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["SeqFormer", "IDOL"])
def test_swin_model_training_step_on_gpu(arch, forward_counter):
    _swin_step(arch)
    assert forward_counter[0] >= 8


@pytest.mark.gpu
def test_swin_graph_replayed_inference_equals_eager_on_gpu():
    torch.manual_seed(5)
    model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cuda:0", **SEQ_TINY, **SMALL_SWIN})).eval()
    clips = T.synthetic_clips(2, 2, 96, 160, "cuda:0", seed=8, num_instances=0)
    graphed = [model([c]) for c in clips]
    assert len(model._graphs) == 1
    model.graph_inference = False
    eager = [model([c]) for c in clips]
    for g, e in zip(graphed, eager):
        assert g["pred_labels"] == e["pred_labels"]
        np.testing.assert_allclose(g["pred_scores"], e["pred_scores"], rtol=1e-5)
        for mg, me in zip(g["pred_masks"], e["pred_masks"]):
            assert float((mg != me).float().mean()) < 1e-3


@pytest.mark.gpu
def test_swin_ddp_wrapper_over_rccl_on_one_gpu():
    """One-rank RCCL group, the wrapper train.py uses (static graph, find_unused_parameters=False): norm0 (res2, never read)
    does not trip it, and a step trains."""
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    port = 29950 + (os.getpid() % 40)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        torch.manual_seed(21)
        model = build_model(get_seqformer_cfg(**{"MODEL.DEVICE": "cuda:0", **SEQ_TINY, **SMALL_SWIN})).train()
        clips = T.synthetic_clips(2, 2, 96, 160, "cuda:0", seed=12, num_instances=2)
        ddp = DistributedDataParallel(model, device_ids=[0], broadcast_buffers=False, find_unused_parameters=False,
                                      static_graph=True, gradient_as_bucket_view=True)
        opt = T.build_optimizer(model)
        table = model.detr.detr.backbone.layers[0].blocks[0].attn.relative_position_bias_table
        before = table.detach().clone()
        losses = [float(T.train_step(ddp, opt, clips)) for _ in range(2)]
        assert all(np.isfinite(losses))
        assert not torch.equal(before, table.detach())
    finally:
        dist.destroy_process_group()
