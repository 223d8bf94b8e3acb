"""Reference checkpoints in, reference checkpoints out: the backbone's names.

Everything but the backbone carries the reference's names already (tests/test_model_ddp.py pins them).  The backbone sits
one wrapper deeper in the reference -- `detr.detr.backbone.0.backbone.<name>` (a Joiner of MaskedBackbone and the position
encoding) where this package has `detr.detr.backbone.<name>` -- and its ResNet carries detectron2's module names:

    reference (detectron2)                   this trunk
    stem.conv1.weight                        stem.0.weight
    stem.conv1.norm.{weight, bias, ..}       stem.1.{..}
    resN.B.convK.weight                      resN.B.convK.weight
    resN.B.convK.norm.{..}                   resN.B.bnK.{..}
    resN.B.shortcut.weight                   resN.B.down.0.weight
    resN.B.shortcut.norm.{..}                resN.B.down.1.{..}

The Swin backbone's names are the reference's: only the prefix differs.  Both maps are pure functions of the key string.
"""
from __future__ import annotations

import re

REFERENCE_PREFIX = "detr.detr.backbone.0.backbone."
LOCAL_PREFIX = "detr.detr.backbone."

_TO_LOCAL = ((re.compile(r"^stem\.conv1\.norm\."), "stem.1."),
             (re.compile(r"^stem\.conv1\."), "stem.0."),
             (re.compile(r"^(res\d+\.\d+)\.conv(\d)\.norm\."), r"\1.bn\2."),
             (re.compile(r"^(res\d+\.\d+)\.shortcut\.norm\."), r"\1.down.1."),
             (re.compile(r"^(res\d+\.\d+)\.shortcut\."), r"\1.down.0."))
_TO_REFERENCE = ((re.compile(r"^stem\.1\."), "stem.conv1.norm."),
                 (re.compile(r"^stem\.0\."), "stem.conv1."),
                 (re.compile(r"^(res\d+\.\d+)\.bn(\d)\."), r"\1.conv\2.norm."),
                 (re.compile(r"^(res\d+\.\d+)\.down\.1\."), r"\1.shortcut.norm."),
                 (re.compile(r"^(res\d+\.\d+)\.down\.0\."), r"\1.shortcut."))


def _sub(name: str, table) -> str:
    for pattern, repl in table:
        new, n = pattern.subn(repl, name, count=1)
        if n:
            return new
    return name


def trunk_key_from_reference(name: str) -> str:
    """a key of detectron2's ResNet (no prefix) -> the key of `ResNetTrunk`; Swin keys and unknown keys unchanged"""
    return _sub(name, _TO_LOCAL)


def trunk_key_to_reference(name: str) -> str:
    """a key of `ResNetTrunk` (no prefix) -> detectron2's; Swin keys and unknown keys unchanged"""
    return _sub(name, _TO_REFERENCE)


def key_from_reference(key: str) -> str:
    """a key of a reference checkpoint -> this package's key"""
    if key.startswith(REFERENCE_PREFIX):
        return LOCAL_PREFIX + trunk_key_from_reference(key[len(REFERENCE_PREFIX):])
    return key


def key_to_reference(key: str) -> str:
    """a key of one of this package's models -> the reference's key"""
    if key.startswith(LOCAL_PREFIX) and not key.startswith(REFERENCE_PREFIX):
        return REFERENCE_PREFIX + trunk_key_to_reference(key[len(LOCAL_PREFIX):])
    return key


def _is_backbone(module) -> bool:
    from ..models.resnet import ResNetTrunk
    from ..models.swin import D2SwinTransformer
    return isinstance(module, (ResNetTrunk, D2SwinTransformer))


def reference_state_dict(model):
    """`model.state_dict()` under the reference's names, in the same order, sharing the tensors: a model trained here loads
    in the reference.  `model` is a SeqFormer / IDOL model, or a bare backbone (keys without a prefix)."""
    bare = _is_backbone(model)
    rename = trunk_key_to_reference if bare else key_to_reference
    items = [(rename(k), v) for k, v in model.state_dict().items()]
    # detectron2's BottleneckBlock registers its shortcut BEFORE conv1, this trunk's block its `down` last: the keys of a
    # block leave in the reference's order (a stable sort: everything else keeps its place)
    block = re.compile(r"^%s(res\d+\.\d+)\.(shortcut\.)?" % ("" if bare else re.escape(REFERENCE_PREFIX)))
    first, order = {}, []
    for i, (k, _) in enumerate(items):
        m = block.match(k)
        if m is None:
            order.append((i, 0, i))
        else:
            order.append((first.setdefault(m.group(1), i), 0 if m.group(2) else 1, i))
    return type(model.state_dict())(items[i] for _, _, i in sorted(order))


def load_reference_checkpoint(model, state, strict: bool = True):
    """Load a reference checkpoint (`state`: a state dict, or a dict with a "model" entry) into `model`: the backbone's
    keys renamed as the module docstring lists, every other key unchanged.  -> what `load_state_dict` returns."""
    if isinstance(state, dict) and "model" in state and isinstance(state["model"], dict):
        state = state["model"]
    rename = trunk_key_from_reference if _is_backbone(model) else key_from_reference
    return model.load_state_dict({rename(k): v for k, v in state.items()}, strict=strict)
