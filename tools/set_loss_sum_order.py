"""How far the order of set_loss.hip's fp32 sums is from float64, against ATen's own order (the multiple
in tests/test_set_loss.py).  CPU only, no library needed.

For every case of tests/test_set_loss.py the fp32 TERMS are ATen's (the element-wise focal terms, the per-(pair, frame)
L1 and GIoU terms of `compose` in fp32); they are then added in float32 in the kernel's order -- a lane of the piece's 256
adds its groups one after the other (four consecutive terms per group where K % 4 == 0, else one), the 64 lanes of a
wave meet in the xor exchange tree 32, 16, .. 1, the four waves are added in order, and the layer's pieces go through the
finishing wave the same way -- and both that sum and ATen's own fp32 sum of the same terms are compared with the float64
`compose`.  Units: absolute error over the column's largest magnitude, as in the test.

    python tools/set_loss_sum_order.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PIECE, MAX_ROWS, THREADS = 4096, 1024, 256
f32 = np.float32


def wave_tree(v):
    """v [..., 64] float32 -> lane 0 of the xor exchange 32, 16, .. 1"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(f32)
    return v[..., 0]


def lanes_then_tree(per_lane_terms, lanes):
    """per_lane_terms: list over lanes of float32 sequences -> the workgroup's (or wave's) sum in the kernel's order"""
    width = max((len(t) for t in per_lane_terms), default=0)
    m = np.zeros((lanes, width), f32)
    for i, t in enumerate(per_lane_terms):
        m[i, :len(t)] = t
    acc = np.zeros(lanes, f32)
    for j in range(width):                                # adding a padded 0 is exact
        acc = (acc + m[:, j]).astype(f32)
    waves = wave_tree(acc.reshape(-1, 64))
    out = f32(0)
    for w in waves:
        out = f32(out + w)
    return out


def kernel_order(focal, l1_terms, giou_terms, lay, clip, qry):
    """focal fp32 [Ld, N, Q, K]; l1_terms / giou_terms fp32 [R, T] -> [Ld, 3] as the two forward launches add them"""
    Ld, N, Q, K = focal.shape
    T = l1_terms.shape[1] if l1_terms.size else 1
    rows = max(1, min(MAX_ROWS, PIECE // K))
    group = 4 if K % 4 == 0 else 1
    out = np.zeros((Ld, 3), f32)
    for l in range(Ld):
        partials = []
        for n in range(N):
            for q0 in range(0, Q, rows):
                nq = min(rows, Q - q0)
                flat = focal[l, n, q0:q0 + nq].reshape(-1)
                groups = flat.reshape(-1, group)
                a = lanes_then_tree([groups[t::THREADS].reshape(-1) for t in range(THREADS)], THREADS)
                sel = [r for r in range(len(lay)) if lay[r] == l and clip[r] == n and q0 <= qry[r] < q0 + nq]
                per_lane = [[[], []] for _ in range(THREADS)]
                for t in range(T):
                    for r in sorted(sel, key=lambda r: qry[r]):
                        idx = t * nq + (qry[r] - q0)
                        per_lane[idx % THREADS][0].append((idx, l1_terms[r, t]))
                        per_lane[idx % THREADS][1].append((idx, giou_terms[r, t]))
                b = lanes_then_tree([np.array([v for _, v in sorted(pl[0])], f32) for pl in per_lane], THREADS)
                c = lanes_then_tree([np.array([v for _, v in sorted(pl[1])], f32) for pl in per_lane], THREADS)
                partials.append((a, b, c))
        partials = np.array(partials, f32)                # the finishing wave: lane j adds partials j, j + 64, ..
        for col in range(3):
            out[l, col] = lanes_then_tree([partials[j::64, col] for j in range(64)], 64)
    return out


def main():
    import test_set_loss as ts
    from vnext_amd.models.criterion import box_cxcywh_to_xyxy, giou_loss
    worst = {}
    for name in ts.CASES:
        case, w, ref = ts.case_and_reference(name)
        logits, boxes, lay, clip, qry, tgt, labels, tgt_boxes, kw = case
        alpha = kw.get("alpha", 0.25)
        aten = ts.compose(*case[:8], **kw)                # ATen's own fp32 sums (CPU)
        onehot = torch.zeros_like(logits)
        onehot[lay, clip, qry, labels[tgt]] = 1
        p = logits.sigmoid()
        ce = F.binary_cross_entropy_with_logits(logits, onehot, reduction="none")
        focal = ce * (1 - (p * onehot + (1 - p) * (1 - onehot))) ** 2.0
        if alpha >= 0:
            focal = (alpha * onehot + (1 - alpha) * (1 - onehot)) * focal
        pred = boxes.transpose(2, 3)[lay, clip, qry]
        want = tgt_boxes[tgt]
        l1_terms = (pred - want).abs().sum(-1)
        giou_terms = giou_loss(box_cxcywh_to_xyxy(pred), box_cxcywh_to_xyxy(want))
        ours = kernel_order(focal.numpy(), l1_terms.numpy(), giou_terms.numpy(), lay.tolist(), clip.tolist(), qry.tolist())
        want64 = ref[0][:, :3].numpy()
        for col, key in enumerate(("focal", "l1", "giou")):
            scale = np.abs(want64[:, col]).max()
            if scale == 0:
                continue
            e_ours = np.abs(ours[:, col].astype(np.float64) - want64[:, col]).max() / scale
            e_aten = np.abs(aten[:, col].double().numpy() - want64[:, col]).max() / scale
            ratio = e_ours / e_aten if e_aten > 0 else float("inf") if e_ours > 0 else 0.0
            print(f"{name:40s} {key:6s} kernel order {e_ours:.3e}  ATen order {e_aten:.3e}  ratio {ratio:.2f}")
            if e_aten > 0:
                worst[key] = max(worst.get(key, 0.0), ratio)
            worst[key + "_abs"] = max(worst.get(key + "_abs", 0.0), e_ours)
    print("worst ratios / errors:", {k: float("%.3g" % v) for k, v in worst.items()})


if __name__ == "__main__":
    main()
