"""Attentive probe: the head of FactorizedVideoClassifier (encoders.py:634-652, `atten_pooler` then
`projection`) as a trainable torch module over frozen tokens.

The classifier builders have no checkpoint for the head; VideoPrism is evaluated with a frozen backbone and
a trained attentive probe.  `AttentiveProbe` runs the head's forward and backward in the library's HIP kernels
(`vp_op_probe_forward` / `vp_op_probe_backward`): the tokens are the encoder's `spatiotemporal_features` and
take no gradient, so each direction is two streaming passes over them.  Loss and optimiser are the user's torch
code; `merge_into` puts the trained head back into a classifier's variables.

Token paddings.  `AttentiveProbe.forward(tokens, paddings)` takes the `paddings` [B, S] of the reference's
AttenTokenPoolingLayer (layers.py:1103-1106, 1 = padded): videos of different lengths, or several clips joined into
one video-level token set, share a batch (`pad_tokens`), and the tokens of padded frames stay out of the pooled
embedding (`token_paddings`).  The kernels skip the padded rows, so a ragged batch costs about what its valid
tokens cost.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _native
from . import params as params_lib


def head_leaf_specs(model_dim: int, num_heads: int, num_classes: int) -> dict[str, tuple[int, ...]]:
    """{path: shape} of the head's leaves: those of params.classifier_leaf_specs outside 'encoder/'."""
    D, H = model_dim, num_heads
    dh = D // H
    pre = "atten_pooler/pooling_attention"
    specs = {"atten_pooler/pooling_attention_query": (1, D), f"{pre}/per_dim_scale/per_dim_scale": (dh,)}
    for q in ("query", "key", "value"):
        specs[f"{pre}/{q}/w"] = (D, H, dh)
        specs[f"{pre}/{q}/b"] = (H, dh)
    specs[f"{pre}/post/w"] = (D, H, dh)
    specs[f"{pre}/post/b"] = (D,)
    specs["atten_pooler/pooling_attention_layer_norm/scale"] = (D,)
    specs["atten_pooler/pooling_attention_layer_norm/bias"] = (D,)
    specs["projection/linear/kernel"] = (D, num_classes)
    specs["projection/linear/bias"] = (num_classes,)
    return specs


def token_paddings(frame_paddings: torch.Tensor, tokens_per_frame: int) -> torch.Tensor:
    """Frame paddings [B, T] (1 = padded frame) -> token paddings [B, T * N] for `spatiotemporal_features`, whose
    tokens are frame-major: token t * N + n is patch n of frame t."""
    if frame_paddings.dim() != 2 or tokens_per_frame < 1:
        raise ValueError(f"frame_paddings must be [B, T] and tokens_per_frame >= 1, got "
                         f"{tuple(frame_paddings.shape)} and {tokens_per_frame}")
    return frame_paddings.repeat_interleave(tokens_per_frame, dim=1)


def pad_tokens(token_sets) -> tuple[torch.Tensor, torch.Tensor]:
    """Token sets [S_i, D] of one dtype, width and device -> (tokens [B, max S_i, D], zero past each set's own
    length, paddings [B, max S_i] fp32, 1 there): the ragged batch `AttentiveProbe.forward` takes."""
    sets = list(token_sets)
    if not sets or any(t.dim() != 2 or t.shape[0] < 1 for t in sets):
        raise ValueError("pad_tokens needs a non-empty list of [S_i, D] tensors with S_i >= 1")
    first = sets[0]
    if any(t.shape[1] != first.shape[1] or t.dtype != first.dtype or t.device != first.device for t in sets):
        raise ValueError("pad_tokens: the token sets must share width, dtype and device")
    S = max(t.shape[0] for t in sets)
    tokens = first.new_zeros((len(sets), S, first.shape[1]))
    paddings = torch.ones((len(sets), S), dtype=torch.float32, device=first.device)
    for b, t in enumerate(sets):
        tokens[b, :t.shape[0]] = t
        paddings[b, :t.shape[0]] = 0.0
    return tokens, paddings


class _ProbeFunction(torch.autograd.Function):
    """logits = head(tokens, paddings; params).  Tokens and paddings take no gradient; the parameters take theirs
    from vp_op_probe_backward(_masked), which reads the workspace the forward filled and is given the forward's
    paddings (None: the unmasked calls)."""

    @staticmethod
    def forward(ctx, tokens, paddings, dims, *leaves):
        B, S, _ = tokens.shape
        tensors = {m: t.detach().contiguous() for (m, _), t in zip(_native.PROBE_LEAVES, leaves)}
        ws = torch.empty(_native.op_probe_workspace_bytes(*dims, B, S), dtype=torch.uint8, device=tokens.device)
        logits = torch.empty((B, dims[2]), dtype=torch.float32, device=tokens.device)
        _native.op_probe_forward(dims, tensors, tokens, logits, None, ws, paddings=paddings)
        ctx.dims, ctx.tokens, ctx.paddings, ctx.tensors, ctx.ws = dims, tokens, paddings, tensors, ws
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        grads = {m: torch.empty_like(t) for m, t in ctx.tensors.items()}
        _native.op_probe_backward(ctx.dims, ctx.tensors, ctx.tokens, dlogits.contiguous().float(), grads, ctx.ws,
                                  paddings=ctx.paddings)
        return (None, None, None) + tuple(grads[m] for m, _ in _native.PROBE_LEAVES)


class AttentiveProbe(torch.nn.Module):
    """The classifier's head over frozen tokens: tokens [B, S, D] (bf16 or fp32, on the GPU) -> logits [B, C] fp32.

    `paddings` [B, S] (bool, integer or floating, on the tokens' device; a token is padded iff its value is > 0.5,
    in any pattern) keeps the padded tokens out of the softmax exactly as the reference's layer does: in a clip with
    a valid token they get probability 0, their contents are never read (NaN and Inf included) and they add nothing
    to any gradient; a clip whose tokens are all padded pools all of them uniformly.  It takes no gradient.

    The parameters are fp32 `nn.Parameter`s named by the reference's paths under 'params', from
    'atten_pooler/pooling_attention_query' to 'projection/linear/bias', in the reference's shapes
    (params.classifier_leaf_specs).  Widths: model_dim a multiple of 128 up to 1536 and of num_heads <= 16.

    Initialisation (nothing in the reference pins a trained head's): biases, per_dim_scale and the LayerNorm scale
    (used as 1 + scale) are zero; every matrix is normal with variance 1 / fan_in (fan_in D for query / key /
    value / projection, H * dh for post); the pooling query is normal with variance 1 / D.  `seed` makes it
    reproducible.

    Fine-tuning the encoder is out of scope: tokens that require a gradient raise NotImplementedError."""

    def __init__(self, model_dim: int, num_heads: int, num_classes: int, device=None, seed: int = 0):
        super().__init__()
        if model_dim < 1 or num_heads < 1 or num_classes < 1 or model_dim % num_heads:
            raise ValueError(f"bad probe dims: model_dim {model_dim}, num_heads {num_heads}, num_classes {num_classes}")
        self.model_dim, self.num_heads, self.num_classes = model_dim, num_heads, num_classes
        rng = np.random.default_rng(seed)
        for name, shape in head_leaf_specs(model_dim, num_heads, num_classes).items():
            leaf = name.rsplit("/", 1)[-1]
            if leaf in ("w", "kernel", "pooling_attention_query"):
                fan_in = shape[1] * shape[2] if name.endswith("post/w") else model_dim
                v = rng.standard_normal(shape).astype(np.float32) / np.float32(math.sqrt(fan_in))
            else:
                v = np.zeros(shape, np.float32)
            self.register_parameter(name, torch.nn.Parameter(torch.from_numpy(v).to(device)))

    @property
    def dims(self) -> tuple[int, int, int]:
        return (self.model_dim, self.num_heads, self.num_classes)

    def _leaves(self):
        return [self._parameters[path] for _, path in _native.PROBE_LEAVES]

    def forward(self, tokens: torch.Tensor, paddings: torch.Tensor | None = None) -> torch.Tensor:
        if tokens.requires_grad:
            raise NotImplementedError("AttentiveProbe trains the head over frozen tokens: the tokens take no "
                                      "gradient (detach them; fine-tuning the encoder is out of scope)")
        if tokens.dim() != 3 or tokens.shape[-1] != self.model_dim:
            raise ValueError(f"tokens must be [B, S, {self.model_dim}], got {tuple(tokens.shape)}")
        if not tokens.is_cuda or tokens.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("tokens must be a bf16 or fp32 tensor on the GPU")
        leaves = self._leaves()
        for (_, path), p in zip(_native.PROBE_LEAVES, leaves):
            if p.device != tokens.device or p.dtype != torch.float32:
                raise ValueError(f"parameter {path} must be fp32 on {tokens.device} (probe.to(device))")
        if paddings is not None:
            if tuple(paddings.shape) != tuple(tokens.shape[:2]):
                raise ValueError(f"paddings must be {tuple(tokens.shape[:2])} like the tokens' [B, S], got "
                                 f"{tuple(paddings.shape)}")
            if paddings.device != tokens.device:
                raise ValueError(f"paddings must be on the tokens' device {tokens.device}, got {paddings.device}")
            paddings = paddings.detach().to(torch.float32).contiguous()
        return _ProbeFunction.apply(tokens.contiguous(), paddings, self.dims, *leaves)

    # ---- the reference's variables ----
    def to_variables(self) -> dict:
        """The head's subtree {'atten_pooler': ..., 'projection': {'linear': ...}} as fp32 NumPy arrays."""
        return params_lib.unflatten({name: p.detach().cpu().numpy().copy() for name, p in self.named_parameters()})

    def merge_into(self, classifier_variables: dict) -> dict:
        """A full {'params': tree} for FactorizedVideoClassifier.apply: the given variables' 'encoder' subtree
        (its leaves are shared, not copied) with this head in place of theirs."""
        tree = classifier_variables.get("params", classifier_variables)
        if "encoder" not in tree:
            raise ValueError("merge_into needs a classifier's variables: no 'encoder' subtree")
        return {"params": dict(self.to_variables(), encoder=tree["encoder"])}

    @classmethod
    def from_variables(cls, variables: dict, num_heads: int, device=None) -> "AttentiveProbe":
        """The inverse of to_variables / merge_into: from a head subtree or a classifier's full variables
        ({'params': tree} or the bare tree).  num_heads is checked against the leaves' shapes."""
        tree = variables.get("params", variables)
        flat = {k: np.asarray(v, dtype=np.float32)
                for k, v in params_lib.flatten({k: v for k, v in tree.items() if k != "encoder"}).items()}
        if "projection/linear/kernel" not in flat:
            raise ValueError("no 'projection/linear/kernel' leaf: not a classifier head's variables")
        D, C = flat["projection/linear/kernel"].shape
        params_lib.validate(flat, head_leaf_specs(D, num_heads, C))
        probe = cls(D, num_heads, C, device=None)
        with torch.no_grad():
            for name, p in probe.named_parameters():
                p.copy_(torch.from_numpy(np.ascontiguousarray(flat[name])))
        return probe.to(device) if device is not None else probe
