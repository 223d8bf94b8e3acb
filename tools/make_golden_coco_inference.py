"""Write tests/golden/coco_inference_idol.npz from the reference's COCO-pretrain evaluation branch (CPU, fp32).

    python tools/make_golden_coco_inference.py --vnext /path/to/VNext

`IDOL.coco_inference` (projects/IDOL/idol/idol.py) and `segmentation_postprocess`
(projects/IDOL/idol/models/segmentation_condInst.py) are cut out of a VNext checkout with `ast` at generation time
(oracle/ref_extract.py; both files import detectron2) and bound to minimal stand-ins for detectron2's `Instances` and
`Boxes` and for `torchvision.ops.batched_nms` (the published algorithm: per-class greedy NMS on IoU, indices in
descending-score order).  The `Boxes` stand-in takes its `clip`, `scale` and `nonempty` from the checkout's
detectron2/structures/boxes.py in the same way.  They run on seeded synthetic network outputs -- 3 images of different sizes reported at
other sizes, Q = 60, K = 6, mask maps 12 x 20, planted objects with near-duplicate boxes -- and the inputs go into the
fixture with the reference's boxes, scores, classes and bit-packed masks.  No reference text is stored; nothing reads
the reference at test time.  Rerunning rewrites byte-identical files.
"""
from __future__ import annotations

import argparse
import io
import os
import sys
import types
import zipfile
from typing import Tuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_extract import extract  # noqa: E402

Q, K, MASK_HW = 60, 6, (12, 20)
IMAGE_SIZES = [(43, 77), (48, 70), (40, 80)]          # before padding to the batch's 48 x 80
OUT_SIZES = [(57, 93), (48, 70), (31, 64)]            # "height" / "width" of the input dicts
MASK_STEP, MASK_SHIFT = 0.125, 0.0127                 # mask logits = int8 * step + shift: small in the file, never 0 after the bilinear resize


class Boxes:
    """detectron2.structures.Boxes: a [n, 4] fp32 tensor and indexing.  `clip`, `scale` and `nonempty`, the members that
    segmentation_postprocess calls, are detectron2's own, bound in main() from the checkout"""

    def __init__(self, tensor):
        self.tensor = tensor.to(torch.float32).reshape(-1, 4)

    def __getitem__(self, item):
        return Boxes(self.tensor[item])


class Instances:
    """detectron2.structures.Instances: fields as attributes, indexing applies to every field"""

    def __init__(self, image_size, **fields):
        object.__setattr__(self, "_image_size", image_size)
        object.__setattr__(self, "_fields", {})
        for k, v in fields.items():
            self._fields[k] = v

    @property
    def image_size(self):
        return self._image_size

    def __setattr__(self, name, value):
        self._fields[name] = value

    def __getattr__(self, name):
        fields = object.__getattribute__(self, "_fields")
        if name not in fields:
            raise AttributeError(name)
        return fields[name]

    def has(self, name):
        return name in self._fields

    def get_fields(self):
        return self._fields

    def __getitem__(self, item):
        return Instances(self._image_size, **{k: v[item] for k, v in self._fields.items()})


def batched_nms_published(boxes, scores, idxs, thr):
    order = torch.argsort(scores, descending=True, stable=True)
    keep = []
    alive = torch.ones(len(order), dtype=torch.bool)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    for a in range(len(order)):
        if not alive[a]:
            continue
        i = order[a]
        keep.append(int(i))
        for b in range(a + 1, len(order)):
            j = order[b]
            if not alive[b] or idxs[i] != idxs[j]:
                continue
            lt, rb = torch.max(boxes[i, :2], boxes[j, :2]), torch.min(boxes[i, 2:], boxes[j, 2:])
            wh = (rb - lt).clamp(min=0)
            inter = wh[0] * wh[1]
            if inter / (area[i] + area[j] - inter) > thr:
                alive[b] = False
    return torch.tensor(keep, dtype=torch.long)


def box_cxcywh_to_xyxy(x):
    c, wh = x[..., :2], x[..., 2:]
    return torch.cat([c - 0.5 * wh, c + 0.5 * wh], -1)


def synthetic_outputs(seed=11, objects=5):
    """-> logits [B, Q, K], boxes [B, Q, 4] (cxcywh), quantised mask logits int8 [B, Q, h, w]"""
    g = torch.Generator().manual_seed(seed)
    B, (h, w) = len(IMAGE_SIZES), MASK_HW
    ys, xs = torch.arange(h)[:, None].float(), torch.arange(w)[None, :].float()
    logits = -4.0 + 0.5 * torch.randn(B, Q, K, generator=g)
    boxes = torch.cat([0.2 + 0.6 * torch.rand(B, Q, 2, generator=g), 0.05 + 0.2 * torch.rand(B, Q, 2, generator=g)], -1)
    masks = -3.0 + 0.5 * torch.randn(B, Q, h, w, generator=g)
    for b in range(B):
        slots = torch.randperm(Q, generator=g).tolist()
        for k in range(objects):
            cls = int(torch.randint(0, K, (1,), generator=g))
            pos = torch.rand(2, generator=g) * torch.tensor([w - 7.0, h - 5.0])
            base = torch.tensor([(pos[0] + 3.5) / w, (pos[1] + 2.5) / h, 7.0 / w, 5.0 / h])
            for d in range(int(torch.randint(1, 4, (1,), generator=g))):      # near-duplicate boxes: what the NMS removes
                q = slots.pop()
                logits[b, q, cls] = 1.5 - 0.6 * d + 0.5 * torch.randn(1, generator=g).item()
                boxes[b, q] = base + 0.012 * d * torch.randn(4, generator=g)
                inside = (xs >= pos[0]) & (xs < pos[0] + 7) & (ys >= pos[1]) & (ys < pos[1] + 5)
                masks[b, q] = torch.where(inside, 3.0, -3.0) + 0.5 * torch.randn(h, w, generator=g)
        # an edge case of segmentation_postprocess: a box that is empty after the clip (wholly left of the image)
        q = slots.pop()
        logits[b, q, 0] = 0.7
        boxes[b, q] = torch.tensor([-0.2, 0.5, 0.1, 0.2])
    mask_q = torch.round(masks / MASK_STEP).clamp(-127, 127).to(torch.int8)
    return logits, boxes, mask_q


def mask_logits(mask_q):
    return torch.from_numpy(np.asarray(mask_q)).float() * MASK_STEP + MASK_SHIFT


def save_npz(path, arrays):
    """np.savez's format with fixed member timestamps, so that a rerun rewrites the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--vnext", required=True, help="root of a VNext checkout (the reference)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    idol = os.path.join(args.vnext, "projects", "IDOL", "idol")
    ns = {"ops": types.SimpleNamespace(batched_nms=batched_nms_published), "box_cxcywh_to_xyxy": box_cxcywh_to_xyxy,
          "Instances": Instances, "Boxes": Boxes}
    for name, fn in extract(os.path.join(args.vnext, "detectron2", "structures", "boxes.py"), ["clip", "scale", "nonempty"],
                            {"Tuple": Tuple}).items():
        setattr(Boxes, name, fn)
    coco_inference = extract(os.path.join(idol, "idol.py"), ["coco_inference"], ns)["coco_inference"]
    postprocess = extract(os.path.join(idol, "models", "segmentation_condInst.py"), ["segmentation_postprocess"],
                          ns)["segmentation_postprocess"]
    logits, boxes, mask_q = synthetic_outputs()
    me = types.SimpleNamespace(mask_on=True)
    results = coco_inference(me, logits.clone(), boxes.clone(), mask_logits(mask_q)[:, :, None], IMAGE_SIZES)
    d = {"pred_logits": logits.numpy(), "pred_boxes": boxes.numpy(), "mask_q8": mask_q.numpy(),
         "mask_scale": np.array([MASK_STEP, MASK_SHIFT], dtype=np.float32),
         "image_sizes": np.array(IMAGE_SIZES), "out_sizes": np.array(OUT_SIZES)}
    for b, (res, (oh, ow)) in enumerate(zip(results, OUT_SIZES)):
        n_before = len(res.scores)
        r = postprocess(res, oh, ow)
        assert tuple(r.image_size) == (oh, ow)
        d[f"i{b}.boxes"] = r.pred_boxes.tensor.numpy()
        d[f"i{b}.scores"] = r.scores.numpy()
        d[f"i{b}.classes"] = r.pred_classes.numpy()
        d[f"i{b}.masks"] = np.packbits(r.pred_masks.numpy().astype(bool), axis=-1)
        print(f"image {b}: {n_before} picked, {len(r.scores)} with a non-empty box, classes {sorted(set(r.pred_classes.tolist()))}, "
              f"masks {tuple(r.pred_masks.shape)}")
    path = os.path.join(args.out, "coco_inference_idol.npz")
    save_npz(path, d)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
