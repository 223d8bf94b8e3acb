"""The ResNet trunk by config (vnext_amd/models/resnet.py: depth, stride placement, refused settings), detectron2's names
for it (vnext_amd/utils/checkpoint.py) and the trunk against detectron2's own ResNet: tests/golden/resnet_d2_r*.npz
(tools/make_golden_resnet.py, float64).  CPU."""
import hashlib
import os

import numpy as np
import pytest
import torch

import resnet_golden_recipe as R
from conftest import GOLDEN_DIR
from vnext_amd import train as T
from vnext_amd.models.resnet import BLOCKS_PER_STAGE, ResNet50Trunk, ResNetTrunk, build_backbone
from vnext_amd.registry import build_model, get_idol_cfg, get_seqformer_cfg
from vnext_amd.utils.checkpoint import REFERENCE_PREFIX, load_reference_checkpoint, reference_state_dict

SEQ_TINY = {"MODEL.DEVICE": "cpu", "MODEL.SeqFormer.ENC_LAYERS": 1, "MODEL.SeqFormer.DEC_LAYERS": 1,
            "MODEL.SeqFormer.NUM_OBJECT_QUERIES": 8, "MODEL.SeqFormer.DIM_FEEDFORWARD": 32, "INPUT.SAMPLING_FRAME_NUM": 2}
IDOL_TINY = {"MODEL.DEVICE": "cpu", "MODEL.IDOL.ENC_LAYERS": 1, "MODEL.IDOL.DEC_LAYERS": 1,
             "MODEL.IDOL.NUM_OBJECT_QUERIES": 8, "MODEL.IDOL.DIM_FEEDFORWARD": 32}
SMALL_SWIN = {"MODEL.BACKBONE.NAME": "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM": 32, "MODEL.SWIN.DEPTHS": [2, 2, 2, 2],
              "MODEL.SWIN.NUM_HEADS": [1, 2, 4, 8], "MODEL.SWIN.WINDOW_SIZE": 7}

# The backbone's state-dict keys of the DEFAULT model at the parent commit (the trunk's own names, `detr.detr.backbone.`
# in front of each in both models), in order: the stem, then per block conv1 bn1 conv2 bn2 conv3 bn3 and, in a stage's first
# block, down.0 down.1.  Written out per block kind; the 265 names follow from the 16 blocks of (3, 4, 6, 3).
_BN = ("weight", "bias", "running_mean", "running_var")
_PARENT_STEM = ["stem.0.weight"] + ["stem.1." + b for b in _BN]
_PARENT_BLOCK = [f"conv{k}.weight" if part == "conv" else f"bn{k}.{part}" for k in (1, 2, 3) for part in ("conv",) + _BN]
_PARENT_DOWN = ["down.0.weight"] + ["down.1." + b for b in _BN]
_PARENT_STAGES = (("res2", 3), ("res3", 4), ("res4", 6), ("res5", 3))
PARENT_BACKBONE_KEYS = _PARENT_STEM + [f"{stage}.{i}.{k}" for stage, n in _PARENT_STAGES for i in range(n)
                                       for k in _PARENT_BLOCK + (_PARENT_DOWN if i == 0 else [])]
# the whole key list of each default model at the parent commit: how many, and sha256 of "\n".join(keys)
PARENT_MODEL_KEYS = {"seqformer": (733, "61150a05d042ff8daaa6467582cee1020922f2af7d2ff772f9eaabcb4ecf306e"), "idol": (619, "829be0e234c1d5177995c1ecde5308f4262882a841465a0066c119f9cf6b1a75")}


def _blocks(trunk):
    return [len(s) for s in (trunk.res2, trunk.res3, trunk.res4, trunk.res5)]


@pytest.mark.parametrize("depth", [50, 101, 152])
def test_blocks_per_stage(depth):
    want = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}[depth]
    assert BLOCKS_PER_STAGE[depth] == want
    with torch.device("meta"):
        trunk = ResNetTrunk(depth)
    assert tuple(_blocks(trunk)) == want
    assert trunk.num_channels == (512, 1024, 2048) and trunk.strides == (8, 16, 32)


def test_depth_101_from_both_cfg_builders():
    idol = build_model(get_idol_cfg(**{"MODEL.RESNETS.DEPTH": 101, **IDOL_TINY}))
    seq = build_model(get_seqformer_cfg(**{"MODEL.RESNETS.DEPTH": 101, **SEQ_TINY}))
    for model in (idol, seq):
        trunk = model.detr.detr.backbone
        assert isinstance(trunk, ResNetTrunk) and sum(_blocks(trunk)) == 33 and trunk.depth == 101
        # FREEZE_AT 2: the stem and res2 frozen, res3 trained
        assert not trunk.stem[0].weight.requires_grad and not trunk.res2[0].conv1.weight.requires_grad
        assert trunk.res3[0].conv1.weight.requires_grad


def test_cfg_without_resnets_node_builds_the_16_block_trunk():
    cfg = get_seqformer_cfg(**SEQ_TINY)
    del cfg.MODEL.RESNETS
    trunk = build_backbone(cfg)
    assert isinstance(trunk, ResNet50Trunk) and sum(_blocks(trunk)) == 16
    assert not trunk.res2[2].conv3.weight.requires_grad and trunk.res3[0].conv1.weight.requires_grad


def test_freeze_at_comes_from_the_backbone_node():
    trunk = build_backbone(get_idol_cfg(**{"MODEL.BACKBONE.FREEZE_AT": 3, **IDOL_TINY}))
    assert not trunk.res3[3].conv3.weight.requires_grad and trunk.res4[0].conv1.weight.requires_grad
    trunk = build_backbone(get_idol_cfg(**{"MODEL.BACKBONE.FREEZE_AT": 0, **IDOL_TINY}))
    assert trunk.stem[0].weight.requires_grad


@pytest.mark.parametrize("arch", ["seqformer", "idol"])
def test_default_model_state_dict_keys_are_the_parents(arch):
    cfg = get_seqformer_cfg(**{"MODEL.DEVICE": "cpu"}) if arch == "seqformer" else get_idol_cfg(**{"MODEL.DEVICE": "cpu"})
    model = build_model(cfg)
    keys = list(model.state_dict().keys())
    assert type(model.detr.detr.backbone).__name__ in ("ResNetTrunk", "ResNet50Trunk")
    assert [k for k in keys if k.startswith("detr.detr.backbone.")] == ["detr.detr.backbone." + k for k in PARENT_BACKBONE_KEYS]
    assert len(PARENT_BACKBONE_KEYS) == 265
    count, sha = PARENT_MODEL_KEYS[arch]
    assert len(keys) == count and hashlib.sha256("\n".join(keys).encode()).hexdigest() == sha


def test_depth_50_trunk_initialises_as_before():
    """same modules in the same order draw the same values from the same seed"""
    torch.manual_seed(11)
    a = ResNet50Trunk()
    torch.manual_seed(11)
    b = ResNetTrunk(50)
    assert list(a.state_dict()) == PARENT_BACKBONE_KEYS == list(b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert torch.equal(torch.rand(4), _after_parent_trunk(11))      # and the generator is left where the parent left it


def _after_parent_trunk(seed):
    """the next draw after the parent's constructor: 53 convolutions' default initialisation, in module order"""
    torch.manual_seed(seed)
    torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    cin = 64
    for mid, cout, n in ((64, 256, 3), (128, 512, 4), (256, 1024, 6), (512, 2048, 3)):
        for i in range(n):
            torch.nn.Conv2d(cin, mid, 1, bias=False), torch.nn.Conv2d(mid, mid, 3, bias=False), torch.nn.Conv2d(mid, cout, 1, bias=False)
            if i == 0:
                torch.nn.Conv2d(cin, cout, 1, bias=False)
            cin = cout
    return torch.rand(4)


def _fixture(name):
    return np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))


def _reference_state(trunk, name):
    """{detectron2 name: the recipe's float64 tensor}, in the fixture's order, digest checked"""
    fx, case = _fixture(name), R.CASES[name]
    shapes = {k: v.shape for k, v in reference_state_dict(trunk).items()}
    state = R.reference_state([(str(k), shapes[str(k)]) for k in fx["state_keys"]], case["seed"])
    assert R.digest(state, R.make_input(case)) == str(fx["digest"]), f"{name}: regenerated weights do not match the fixture"
    return fx, case, state


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_keys_and_round_trip(name):
    fx = _fixture(name)
    trunk = ResNetTrunk(R.CASES[name]["depth"])
    ref_keys = [str(k) for k in fx["state_keys"]]
    assert [k for k in reference_state_dict(trunk)] == ref_keys
    # a bare trunk loads detectron2's names, strictly
    _, _, state = _reference_state(trunk, name)
    result = load_reference_checkpoint(trunk.double(), state, strict=True)
    assert list(result.missing_keys) == [] and list(result.unexpected_keys) == []
    assert torch.equal(trunk.res3[0].down[1].running_var, state["res3.0.shortcut.norm.running_var"])
    assert torch.equal(trunk.stem[1].running_mean, state["stem.conv1.norm.running_mean"])
    assert torch.equal(trunk.res4[1].bn2.weight, state["res4.1.conv2.norm.weight"])
    # round trip: every tensor comes back
    torch.manual_seed(3)
    other = ResNetTrunk(R.CASES[name]["depth"]).double()
    load_reference_checkpoint(other, {"model": reference_state_dict(trunk)})
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in trunk.state_dict().items())


@pytest.mark.parametrize("arch,name", [("idol", "resnet_d2_r50"), ("idol", "resnet_d2_r101"), ("seqformer", "resnet_d2_r101")])
def test_model_loads_a_reference_checkpoint_strictly(arch, name):
    depth = R.CASES[name]["depth"]
    if arch == "idol":
        model = build_model(get_idol_cfg(**{"MODEL.RESNETS.DEPTH": depth, **IDOL_TINY}))
    else:
        model = build_model(get_seqformer_cfg(**{"MODEL.RESNETS.DEPTH": depth, **SEQ_TINY}))
    own = model.state_dict()
    ref = reference_state_dict(model)
    ref_keys = [str(k) for k in _fixture(name)["state_keys"]]
    assert [k for k in ref if k.startswith(REFERENCE_PREFIX)] == [REFERENCE_PREFIX + k for k in ref_keys]
    # a checkpoint as the reference writes it: the fixture's keys under the reference's prefix + the model's other keys
    ckpt = {REFERENCE_PREFIX + k: torch.full_like(ref[REFERENCE_PREFIX + k], 0.25) for k in ref_keys}
    ckpt.update({k: torch.full_like(v, 0.5) for k, v in own.items() if not k.startswith("detr.detr.backbone.")})
    result = load_reference_checkpoint(model, {"model": ckpt}, strict=True)
    assert list(result.missing_keys) == [] and list(result.unexpected_keys) == []
    assert float(model.detr.detr.backbone.res5[2].bn3.running_var.mean()) == 0.25
    # the round trip restores every tensor
    torch.manual_seed(5)
    fresh = {k: torch.randn_like(v) if v.is_floating_point() else v.clone() for k, v in own.items()}
    model.load_state_dict(fresh)
    fresh = {k: v.clone() for k, v in model.state_dict().items()}      # (keys that share a tensor hold the last one loaded)
    saved = {k: v.clone() for k, v in reference_state_dict(model).items()}
    model.load_state_dict({k: torch.zeros_like(v) for k, v in own.items()})
    load_reference_checkpoint(model, saved)
    assert all(torch.equal(v, fresh[k]) for k, v in model.state_dict().items())


def test_swin_keys_only_lose_the_prefix():
    model = build_model(get_seqformer_cfg(**{**SEQ_TINY, **SMALL_SWIN}))
    own = list(model.state_dict())
    ref = list(reference_state_dict(model))
    assert [k.replace(REFERENCE_PREFIX, "detr.detr.backbone.") for k in ref] == own
    assert any(k.startswith(REFERENCE_PREFIX + "layers.0.blocks.0.attn.") for k in ref)
    result = load_reference_checkpoint(model, {k: v.clone() for k, v in reference_state_dict(model).items()})
    assert list(result.missing_keys) == [] and list(result.unexpected_keys) == []


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_outputs_against_detectron2(name):
    trunk = ResNetTrunk(R.CASES[name]["depth"]).double().eval()
    fx, case, state = _reference_state(trunk, name)
    load_reference_checkpoint(trunk, state)
    with torch.no_grad():
        outs = trunk(R.make_input(case))
    for out, key in zip(outs, R.OUTPUTS):
        want = torch.from_numpy(fx[key])
        assert out.shape == want.shape
        err = float((out - want).abs().max() / want.abs().max())
        assert err <= 1e-9, f"{name} {key}: {err:.3e}"


def test_stride_in_1x1_moves_the_stride():
    cfg = get_idol_cfg(**{"MODEL.RESNETS.STRIDE_IN_1X1": True, **IDOL_TINY})
    with torch.device("meta"):
        moved, default = build_backbone(cfg), build_backbone(get_idol_cfg(**IDOL_TINY))
    assert moved.res3[0].conv1.stride == (2, 2) and moved.res3[0].conv2.stride == (1, 1)
    assert default.res3[0].conv1.stride == (1, 1) and default.res3[0].conv2.stride == (2, 2)
    assert moved.res3[0].down[0].stride == (2, 2) and moved.res3[1].conv1.stride == (1, 1)
    assert moved.res2[0].conv1.stride == (1, 1)
    x = torch.randn(1, 3, 32, 48)
    assert [tuple(o.shape) for o in ResNetTrunk(50, True).eval()(x)] == [(1, 512, 4, 6), (1, 1024, 2, 3), (1, 2048, 1, 2)]


@pytest.mark.parametrize("key,value", [("NORM", "BN"), ("RES5_DILATION", 2), ("NUM_GROUPS", 32), ("DEPTH", 34),
                                       ("DEPTH", 18), ("WIDTH_PER_GROUP", 8), ("RES2_OUT_CHANNELS", 64),
                                       ("STEM_OUT_CHANNELS", 32), ("DEFORM_ON_PER_STAGE", [False, True, True, True]),
                                       ("OUT_FEATURES", ["res4"])])
def test_refused_settings_name_their_key(key, value):
    for make, tiny in ((get_idol_cfg, IDOL_TINY), (get_seqformer_cfg, SEQ_TINY)):
        with pytest.raises(ValueError, match="MODEL.RESNETS." + key):
            build_backbone(make(**{"MODEL.RESNETS." + key: value, **tiny}))


def test_fused_glue_switch():
    model = build_model(get_idol_cfg(**IDOL_TINY))
    trunk = model.detr.detr.backbone
    keys = list(model.state_dict())
    assert trunk.fused_glue is False
    T.enable_fused_resnet_glue(model)
    assert trunk.fused_glue is True and list(model.state_dict()) == keys
    # CPU tensors keep the eager chain whatever the switch says
    x = torch.randn(1, 3, 32, 32)
    trunk.eval()
    with torch.no_grad():
        on = trunk(x)
        T.enable_fused_resnet_glue(model, False)
        off = trunk(x)
    assert trunk.fused_glue is False and all(torch.equal(a, b) for a, b in zip(on, off))
    swin = build_model(get_seqformer_cfg(**{**SEQ_TINY, **SMALL_SWIN}))
    with pytest.raises(ValueError, match="ResNet"):
        T.enable_fused_resnet_glue(swin)
