"""Both deformable transformers at the models' width, forward + backward, against float64 (tests/model_grad_harness.py).

Geometry: d_model 256, 8 heads, 4 levels x 4 points, dim_feedforward 1024, 1 encoder and 2 decoder layers, 300 queries, box
refinement on.  The 192x320 pyramid (24,40) ... (3,5) gives 1 275 queries per frame: the encoder takes the tile-fed grad_value
path and the slab kernels (Lq >= 1024), the decoder the self-decoding grad_value kernel and the paired backward (Lq = 300).
SeqFormer runs 2 clips x 5 frames, IDOL 4 images; the second clip / image is padded on the right and at the bottom.  One more
SeqFormer case runs bench.py's 360p pyramid (48,80) ... (6,10) with one clip of 5 frames.

Three runs from the same weights, inputs and upstream gradients G_k (loss = sum_k <G_k, out_k>): (a) the product path on the
GPU, (b) the same on the GPU with every fused path off (ATen + F.grid_sample), (c) float64 on the CPU with the same stand-ins.
Every output, input gradient and parameter gradient is compared by name with e = ||g - g64||_F / ||g64||_F.  A tensor passes
when e_a <= K * e_b + EPS and e_a <= CAP: the ratio to the ATen path separates a kernel's error from fp32's own (GEMM
summation order, samples whose fp32 and fp64 locations straddle a pixel edge), the cap bounds it absolutely.

e_b is the worst of run (b) and three twins of it whose weights are nudged by one fp32 ulp (model_grad_harness.baseline_errors):
a sample whose fp32 and fp64 locations straddle a pixel edge puts an O(1) error into one row of grad_offsets, and (a) and
(b) draw such samples independently.  With one baseline run IDOL's decoder failed the ratio on a correct kernel:
sampling_offsets.bias of its first layer, e_a 8.2e-3 against e_b 3.6e-6.  Every fused MSDA backward of that run, recomputed
in float64 from its own fp32 inputs, agreed within 1.1e-6.

Measured on the MI355X (largest e in each group; "input" = the src / pos / query_embed gradients):

    fp32      seqformer 2x5          idol 4                 seqformer 360p 1x5
              e_a      e_b           e_a      e_b           e_a      e_b
    encoder   1.5e-4   5.1e-4        2.0e-4   1.1e-3        9.7e-4   9.5e-4
    decoder   4.9e-3   4.9e-3        8.2e-3   8.2e-3        2.7e-3   1.8e-2
    input     2.0e-4   5.8e-4        2.7e-3   3.0e-3        1.2e-3   1.7e-2
    output    1.3e-6   1.5e-6        1.3e-6   1.7e-6        3.0e-6   3.8e-6
    largest e_a / e_b: 1.2, 1.0, 2.0

    bf16      e_a      e_b           e_a      e_b           e_a      e_b
    encoder   1.7e-1   1.8e-1        1.6e-1   1.7e-1        1.7e-1   1.9e-1
    decoder   4.0e-1   3.7e-1        5.2e-1   5.2e-1        7.3e-1   7.3e-1
    input     3.1e-1   3.2e-1        3.4e-1   3.9e-1        7.3e-1   7.1e-1
    output    1.9e-2   2.1e-2        2.1e-2   2.3e-2        4.9e-2   5.0e-2
    largest e_a / e_b: 1.7 (seqformer_360p: 1.4; idol: 1.3)

The largest errors sit in the sampling_offsets and reference_points gradients, which only reach the loss through sample
locations.  Caps: FP32_CAP 5e-2 (6x the largest e_a, 8.2e-3), BF16_CAP 1.0 (1.4x the largest, 0.73).  BF16_K 4 and
BF16_EPS 1e-4 leave the unperturbed bf16 runs a margin of 2.3x.
"""
import pytest
import torch

import model_grad_harness as H

FP32_K, FP32_EPS, FP32_CAP = 4.0, 1e-6, 5e-2
BF16_K, BF16_EPS, BF16_CAP = 4.0, 1e-4, 1.0

CASES = {"seqformer": ("seqformer", 2, 5, H.PYRAMID_192P), "idol": ("idol", 4, 1, H.PYRAMID_192P),
         "seqformer_360p": ("seqformer", 1, 5, H.PYRAMID_360P)}
_cache = {}


def _case(name):
    """(kind, master weights, inputs, reference run (c)); built once per process."""
    if name not in _cache:
        kind, clips, frames, pyramid = CASES[name]
        master = H.build(kind, frames, seed=11)
        inputs = H.make_inputs(kind, clips, frames, pyramid, seed=11)
        _cache[name] = (kind, master, inputs, H.reference(kind, master, inputs))
    return _cache[name]


def _baseline(name, autocast):
    """e_b per tensor (model_grad_harness.baseline_errors), once per case and mode; none of the product path's entry points
    may be called by the baseline."""
    key = (name, "b", autocast)
    if key not in _cache:
        kind, master, inputs, ref = _case(name)
        with H.counting_launches() as counts:
            _cache[key] = H.baseline_errors(kind, master, inputs, ref, autocast)
        torch.cuda.synchronize()
        called = {k: v for k, v in counts.items() if k in H.ENTRY_POINTS}
        assert not called, f"the ATen baseline reached fused kernels: {called}"
    return _cache[key]


def _product(name, autocast):
    kind, master, inputs, ref = _case(name)
    return H.step(kind, master, inputs, ref["G"], "cuda:0", torch.float32, autocast=autocast)


def _report(name, tag, e_a, e_b):
    ratio = sorted(e_a, key=lambda n: e_a[n] / max(e_b[n], 1e-30))[-3:]
    print(f"\n[{name} {tag}] worst e_a {H.worst(e_a)} e_b {H.worst(e_b)}\n{H.table(e_a, e_b)}\n  largest e_a / e_b: "
          + ", ".join(f"{n} {e_a[n]:.2e}/{e_b[n]:.2e}" for n in ratio))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_gradients_match_float64(name):
    kind = CASES[name][0]
    _, _, _, ref = _case(name)
    e_b = _baseline(name, False)
    with H.counting_launches() as counts:
        run = _product(name, False)
    torch.cuda.synchronize()
    expected = H.expected_calls(kind)
    got = {k: counts.get(k, 0) for k in expected}
    assert got == expected, f"kernel launches {got}, the layer structure implies {expected}"
    e_a = H.errors(run, ref)
    _report(name, "fp32", e_a, e_b)
    bad = H.violations(e_a, e_b, FP32_K, FP32_EPS, FP32_CAP)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bf16_autocast_gradients_match_float64(name):
    _, _, _, ref = _case(name)
    e_b = _baseline(name, True)
    e_a = H.errors(_product(name, True), ref)      # (step() checks: same Parameter objects, fp32, each with its .grad)
    _report(name, "bf16", e_a, e_b)
    bad = H.violations(e_a, e_b, BF16_K, BF16_EPS, BF16_CAP)
    assert not bad, bad


PERTURBED = [(name, fn) for name in ("seqformer", "idol") for fn in sorted(H.FUNCTIONS)
             if CASES[name][0] == "seqformer" or fn not in ("MSDeformAttnFunction", "_TimeWeightedSum")]
# Perturbations the comparison cannot tell from the location noise above (measured: largest e_a / e_b over all tensors, against
# K = 4).  Their cases still run, check that the perturbed backward was called, and print the numbers.
NOT_SEPARABLE = {
    ("idol", "_AddDropoutLayerNorm", False): 3.1, ("idol", "_QuerySelfAttention", False): 2.3,
    ("seqformer", "MSDeformAttnFunction", True): 1.7, ("seqformer", "MSDeformAttnFusedFunction", True): 1.7,
    ("seqformer", "_AddDropoutLayerNorm", True): 1.2, ("seqformer", "_BiasReluDropout", True): 1.3,
    ("seqformer", "_QuerySelfAttention", True): 1.7, ("seqformer", "_TimeWeightedSum", True): 1.7,
    ("idol", "MSDeformAttnFusedFunction", True): 1.4, ("idol", "_AddDropoutLayerNorm", True): 1.4,
    ("idol", "_BiasReluDropout", True): 1.4, ("idol", "_QuerySelfAttention", True): 1.4,
}


@pytest.mark.gpu
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,fn", PERTURBED)
def test_a_perturbed_backward_fails_the_comparison(name, fn, autocast):
    """The gradient of the Function's first input scaled by 1.01 (bf16: 1.10) on the first batch element, in one call: the
    comparison above must report it -- except for the cases in NOT_SEPARABLE, where the measured effect stays inside the
    noise a correct kernel shows."""
    _, _, _, ref = _case(name)
    e_b = _baseline(name, autocast)
    with H.perturbed_backward(H.FUNCTIONS[fn], 1.10 if autocast else 1.01) as done:
        run = _product(name, autocast)
    assert done[0] == 1, f"{fn}: the product path never ran its backward"
    e_a = H.errors(run, ref)
    k, eps, cap = (BF16_K, BF16_EPS, BF16_CAP) if autocast else (FP32_K, FP32_EPS, FP32_CAP)
    bad = H.violations(e_a, e_b, k, eps, cap)
    worst = max(bad, key=lambda n: bad[n][0] / max(k * bad[n][1] + eps, 1e-30)) if bad else None
    print(f"\n[{name} {fn} {'bf16' if autocast else 'fp32'}] {len(bad)} tensors flagged; worst {worst} "
          f"{bad.get(worst)}; largest e_a / e_b {max(e_a[n] / max(e_b[n], 1e-30) for n in e_a):.2f}")
    if (name, fn, autocast) not in NOT_SEPARABLE:
        assert bad, f"{fn}: a {'10' if autocast else '1'} % error in one call's gradient went unnoticed"
