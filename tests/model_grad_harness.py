"""Shared harness of the composed-gradient tests (test_transformer.py's fixture gradients, test_model_gradients.py): both
deformable transformers at the models' width, one backward from seeded upstream gradients, three ways.

  (a) the product path: GPU, every fused kernel the geometry reaches;
  (b) the ATen baseline: GPU, same dtype, every fused path switched off and MSDA through F.grid_sample;
  (c) the reference: CPU, float64, with the same stand-ins.

The loss is sum_k <G_k, out_k> over the outputs the detector consumes (hs, hs_box, memory, init_ref and the per-layer box
predictions).  A run returns every output, every input gradient and every parameter gradient, keyed by name, as float64 CPU
tensors.  A plain module, not a conftest: the test files import it."""
from __future__ import annotations

import contextlib
import copy

import torch

from vnext_amd import _lib
from vnext_amd.models.idol_transformer import DeformableTransformer as IdolTransformer
from vnext_amd.models.seqformer_transformer import DeformableTransformer as SeqTransformer
from vnext_amd.ops import decoder_glue, fused_ffn, fused_norm, self_attention
from vnext_amd.ops.functions import MSDeformAttnFunction, MSDeformAttnFusedFunction
from vnext_amd.ops.modules import ms_deform_attn as msda_module
from vnext_amd.ops.modules.ms_deform_attn import _MSDeformAttnBase

C, HEADS, LEVELS, POINTS, FFN, ENC, DEC, QUERIES = 256, 8, 4, 4, 1024, 1, 2, 300
PYRAMID_192P = ((24, 40), (12, 20), (6, 10), (3, 5))        # a 192x320 frame: 1 275 queries per frame
PYRAMID_360P = ((48, 80), (24, 40), (12, 20), (6, 10))      # bench.py's 360p frame: 5 100 queries per frame


def grid_sample_function():
    """Differentiable stand-in for the HIP op (oracle/msda_torch_fallback.py; tests only)."""
    from oracle.msda_torch_fallback import msda_grid_sample

    class Fn:
        @staticmethod
        def apply(value, shapes, lsi, loc, attn, step):
            return msda_grid_sample(value, shapes, loc, attn)
    return Fn


@contextlib.contextmanager
def aten_baseline(model=None):
    """Every fused path of the transformers off (all are read at call time), MSDA through F.grid_sample."""
    saved = [(self_attention, "ENABLE"), (decoder_glue, "ENABLE"), (fused_ffn, "ENABLE_FFN"),
             (fused_ffn, "ENABLE_MASKED_LINEAR"), (fused_norm, "fused_applies"), (msda_module, "MSDeformAttnFunction")]
    old = [getattr(o, n) for o, n in saved]
    prologue = [(m, m.fused_prologue) for m in (model.modules() if model is not None else ()) if isinstance(m, _MSDeformAttnBase)]
    try:
        self_attention.ENABLE = decoder_glue.ENABLE = False
        fused_ffn.ENABLE_FFN = fused_ffn.ENABLE_MASKED_LINEAR = False
        fused_norm.fused_applies = lambda *a, **k: False
        msda_module.MSDeformAttnFunction = grid_sample_function()
        for m, _ in prologue:
            m.fused_prologue = False
        yield
    finally:
        for (o, n), v in zip(saved, old):
            setattr(o, n, v)
        for m, v in prologue:
            m.fused_prologue = v


# ------------------------------------------------------------------------------------------------------------------ kernels
ENTRY_POINTS = ("vnx_msda_fused_forward", "vnx_msda_fused_backward", "vnx_msda_forward", "vnx_msda_backward",
                "vnx_add_dropout_layernorm_forward", "vnx_add_dropout_layernorm_backward",
                "vnx_bias_relu_dropout_forward", "vnx_bias_relu_dropout_backward",
                "vnx_query_self_attention_forward", "vnx_query_self_attention_backward",
                "vnx_refine_boxes_forward", "vnx_refine_boxes_backward",
                "vnx_time_weighted_sum_forward", "vnx_time_weighted_sum_backward")


def expected_calls(kind, enc=ENC, dec=DEC):
    """Launches of each entry point in one forward + backward, from the layer structure (forward count == backward count).

    SeqFormer encoder layer: fused MSDA, masked value projection, FFN, 2 LayerNorm passes.  Its first decoder layer: plain MSDA
    (one set of offsets shared by the frames), 2 query self-attentions, 5 LayerNorm passes (norm1_box broadcasts over the
    frames: plain torch), 3 in-place passes (value projection, 2 FFNs), refine_boxes, time_weighted_sum.  A later decoder
    layer: fused MSDA, 6 LayerNorm passes, otherwise the same.  IDOL: fused MSDA everywhere; a decoder layer has one query
    self-attention, 3 LayerNorm passes, value projection + FFN and refine_boxes."""
    if kind == "seqformer":
        per = dict(msda_fused=enc + dec - 1, msda=1, add_dropout_layernorm=2 * enc + 5 + 6 * (dec - 1),
                   bias_relu_dropout=2 * enc + 3 * dec, query_self_attention=2 * dec, refine_boxes=dec,
                   time_weighted_sum=dec)
    else:
        per = dict(msda_fused=enc + dec, msda=0, add_dropout_layernorm=2 * enc + 3 * dec, bias_relu_dropout=2 * enc + 2 * dec,
                   query_self_attention=dec, refine_boxes=dec, time_weighted_sum=0)
    return {f"vnx_{k}_{d}": v for k, v in per.items() for d in ("forward", "backward")}


@contextlib.contextmanager
def counting_launches():
    """Counts every C-ABI call made through vnext_amd._lib.lib() inside the block (as test_swin.py's forward_counter)."""
    lib, real = _lib.lib(), _lib.lib
    counts = {}

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("vnx_"):
                return fn

            def call(*args):
                counts[name] = counts.get(name, 0) + 1
                return fn(*args)
            return call
    _lib.lib = lambda: Counting()
    try:
        yield counts
    finally:
        _lib.lib = real


# ------------------------------------------------------------------------------------------------------------------ builds
def _box_heads(n, width):
    return torch.nn.ModuleList([torch.nn.Sequential(torch.nn.Linear(width, width), torch.nn.ReLU(), torch.nn.Linear(width, width),
                                                    torch.nn.ReLU(), torch.nn.Linear(width, 4)) for _ in range(n)])


def build(kind, frames=1, seed=0):
    """The transformer at the models' width with box refinement, in train() mode with every dropout at 0 (nn.MultiheadAttention's
    included): the constructors' initialisation plus a seeded 0.05 * randn on every parameter -- _reset_parameters zeroes
    sampling_offsets.weight and attention_weights, which would leave whole gradient paths at zero.  fp32, CPU."""
    torch.manual_seed(seed)
    common = dict(d_model=C, nhead=HEADS, num_encoder_layers=ENC, num_decoder_layers=DEC, dim_feedforward=FFN, dropout=0.0,
                  return_intermediate_dec=True, num_feature_levels=LEVELS, dec_n_points=POINTS, enc_n_points=POINTS)
    tr = SeqTransformer(num_frames=frames, **common) if kind == "seqformer" else IdolTransformer(**common)
    tr.decoder.bbox_embed = _box_heads(DEC, C)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in tr.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
    for m in tr.modules():
        if isinstance(m, torch.nn.MultiheadAttention):
            assert m.dropout == 0.0
        if isinstance(m, torch.nn.Dropout):
            assert m.p == 0.0
    return tr.train()


def make_inputs(kind, clips, frames, pyramid, seed=0):
    """srcs / pos per level, padding masks (the second clip / image padded on the right and at the bottom), query_embed: fp32."""
    gen = torch.Generator().manual_seed(seed + 2)
    lead = (clips, frames) if kind == "seqformer" else (clips,)
    srcs = [torch.randn(*lead, C, h, w, generator=gen) for h, w in pyramid]
    poss = [torch.randn(*lead, C, h, w, generator=gen) for h, w in pyramid]
    masks = []
    for h, w in pyramid:
        m = torch.zeros(*lead, h, w, dtype=torch.bool)
        if clips > 1:
            m[1, ..., h - max(1, h // 4):, :] = True
            m[1, ..., :, w - max(1, w // 4):] = True
        masks.append(m)
    return dict(srcs=srcs, poss=poss, masks=masks, query_embed=torch.randn(QUERIES, 2 * C, generator=gen))


def outputs(kind, tr, srcs, masks, poss, query_embed):
    """What the detector consumes of one transformer call; `boxes` are the layers' box predictions (inter_boxes)."""
    if kind == "seqformer":
        hs, hs_box, memory, init_ref, _, boxes, _, _ = tr(srcs, masks, poss, query_embed)
        return dict(hs=hs, hs_box=hs_box, memory=memory, init_ref=init_ref, boxes=boxes)
    hs, memory, init_ref, _, _, boxes, _ = tr(srcs, masks, poss, query_embed)
    return dict(hs=hs, memory=memory, init_ref=init_ref, boxes=boxes)


def upstream(outs, seed=0):
    gen = torch.Generator().manual_seed(seed + 3)
    return {k: torch.randn(v.shape, generator=gen) for k, v in outs.items()}


def step(kind, master, inputs, grads, device, dtype, autocast=False, baseline=False):
    """One forward + backward of a copy of `master` on `device` in `dtype` -> {name: float64 CPU tensor} of the outputs
    ("out.*"), the input gradients ("grad.src{i}", "grad.pos{i}", "grad.query_embed") and the parameter gradients
    ("grad.<parameter>"); parameters without a gradient are left out.  `grads`: the G_k (or None: drawn from the outputs
    of this run, returned under "G")."""
    tr = copy.deepcopy(master).to(device=device, dtype=dtype).train()
    params = dict(tr.named_parameters())
    srcs = [s.to(device, dtype).requires_grad_(True) for s in inputs["srcs"]]
    poss = [p.to(device, dtype).requires_grad_(True) for p in inputs["poss"]]
    masks = [m.to(device) for m in inputs["masks"]]
    query_embed = inputs["query_embed"].to(device, dtype).requires_grad_(True)
    ctx = aten_baseline(tr) if baseline else contextlib.nullcontext()
    with ctx:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            outs = outputs(kind, tr, srcs, masks, poss, query_embed)
        if grads is None:
            grads = upstream(outs)
        wide = torch.float64 if dtype == torch.float64 else torch.float32      # (under autocast: the outputs' own dtype may be 16-bit)
        sum((grads[k].to(device, wide) * v.to(wide)).sum() for k, v in outs.items()).backward()
    after = dict(tr.named_parameters())
    assert set(after) == set(params) and all(after[n] is params[n] for n in params), "parameters were swapped out"
    assert all(p.dtype == dtype for p in params.values()), "a parameter changed dtype"
    res = {f"out.{k}": v.detach().double().cpu() for k, v in outs.items()}
    for i, (s, p) in enumerate(zip(srcs, poss)):
        res[f"grad.src{i}"], res[f"grad.pos{i}"] = s.grad.double().cpu(), p.grad.double().cpu()
    res["grad.query_embed"] = query_embed.grad.double().cpu()
    res.update({f"grad.{n}": p.grad.double().cpu() for n, p in params.items() if p.grad is not None})
    res["G"] = grads
    return res


def nudged(master, seed):
    """`master` with every parameter moved by about one fp32 ulp (relative 2^-23 * randn): the same function to fp32
    precision, other rounding upstream of every sampling location."""
    twin = copy.deepcopy(master)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in twin.parameters():
            p.add_(p * torch.randn(p.shape, generator=gen) * 2.0 ** -23)
    return twin


def baseline_errors(kind, master, inputs, ref, autocast, twins=3):
    """e_b per tensor: the largest error of the ATen baseline (b) over `master` and `twins` nudged copies of it.

    A bilinear sample's gradient with respect to its location jumps at every pixel edge.  A sample whose fp32 and fp64
    locations straddle an edge puts an O(1) error into one row of grad_offsets, and from there into sampling_offsets, the
    query and everything upstream of it -- up to 1e-2 relative in a decoder's sampling_offsets.bias, where a few hundred
    thousand samples give about one such sample per run.  Which samples straddle depends on the last bit of every
    activation upstream, so (a) and (b) draw them independently; one baseline run alone may draw none where (a) drew one.
    The worst of a few twins measures the noise a correct kernel may show; a kernel error in one batch element is not of
    that kind."""
    runs = [master] + [nudged(master, 1000 + i) for i in range(twins)]
    worst = None
    for m in runs:
        e = errors(step(kind, m, inputs, ref["G"], "cuda:0", torch.float32, autocast=autocast, baseline=True), ref)
        worst = e if worst is None else {n: max(worst[n], e[n]) for n in e}
    return worst


def reference(kind, master, inputs, grads=None):
    """Run (c): float64 on the CPU, MSDA through F.grid_sample."""
    with aten_baseline():
        return step(kind, master, inputs, grads, "cpu", torch.float64)


# ------------------------------------------------------------------------------------------------------------------ compare
def rel_err(got, want, scale=None):
    """||got - want||_F / ||scale||_F, scale = want by default (0 when both are zero)."""
    num = float(torch.linalg.vector_norm(got - want))
    den = float(torch.linalg.vector_norm(want if scale is None else scale))
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def _scale(name, ref):
    # time_attention_weights.bias: its gradient is zero in exact arithmetic (the softmax over the frames does not see a shift),
    # both sides hold rounding only -- measured against the gradient of the same Linear's weight instead
    if name.endswith("time_attention_weights.bias"):
        return ref[name[:-len("bias")] + "weight"]
    return None


def errors(run, ref):
    """{name: relative error} over the names of `ref`; a name missing from either side fails."""
    keys_run = {k for k in run if k != "G"}
    keys_ref = {k for k in ref if k != "G"}
    assert keys_run == keys_ref, f"missing {sorted(keys_ref - keys_run)}, extra {sorted(keys_run - keys_ref)}"
    for k in keys_ref:
        assert run[k].shape == ref[k].shape, k
    return {k: rel_err(run[k], ref[k], _scale(k, ref)) for k in sorted(keys_ref)}


def violations(e_a, e_b, k, eps, cap):
    """Names for which the product path is not within k times the ATen path's error (+ eps) or above the absolute cap."""
    bad = {}
    for n in e_a:
        if not (e_a[n] <= k * e_b[n] + eps and e_a[n] <= cap):
            bad[n] = (e_a[n], e_b[n])
    return bad


def group(name):
    """encoder / decoder / input / output: the rows of the summary table."""
    if name.startswith("out."):
        return "output"
    if name.startswith("grad.encoder.") or name == "grad.level_embed":
        return "encoder"
    if name.startswith("grad.decoder.") or name.startswith("grad.reference_points."):
        return "decoder"
    return "input"


def summary(e_a, e_b):
    out = {}
    for n in e_a:
        g = group(n)
        a, b = out.get(g, (0.0, 0.0))
        out[g] = (max(a, e_a[n]), max(b, e_b[n]))
    return out


@contextlib.contextmanager
def perturbed_backward(fn_cls, factor):
    """`fn_cls.backward` with the gradient of its first tensor input scaled by `factor` on the first batch element, in the
    first call only.  Yields a list holding the number of calls perturbed."""
    real = fn_cls.__dict__["backward"]
    inner = real.__func__ if isinstance(real, staticmethod) else real
    done = [0]

    def backward(ctx, *grad_outputs):
        grads = list(inner(ctx, *grad_outputs))
        if not done[0]:
            assert isinstance(grads[0], torch.Tensor), f"{fn_cls.__name__}: no gradient for the first input"
            grads[0] = grads[0].clone()
            grads[0][0] *= factor
            done[0] += 1
        return tuple(grads)
    fn_cls.backward = staticmethod(backward)
    try:
        yield done
    finally:
        fn_cls.backward = real


FUNCTIONS = {"_AddDropoutLayerNorm": fused_norm._AddDropoutLayerNorm, "_BiasReluDropout": fused_ffn._BiasReluDropout,
             "_QuerySelfAttention": self_attention._QuerySelfAttention, "_RefineBoxes": decoder_glue._RefineBoxes,
             "_TimeWeightedSum": decoder_glue._TimeWeightedSum, "MSDeformAttnFunction": MSDeformAttnFunction,
             "MSDeformAttnFusedFunction": MSDeformAttnFusedFunction}


def table(e_a, e_b):
    return "\n".join(f"{g:8s} e_a {a:.2e}  e_b {b:.2e}" for g, (a, b) in sorted(summary(e_a, e_b).items()))


def worst(e):
    n = max(e, key=e.get)
    return n, e[n]

