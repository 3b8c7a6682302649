"""Training the classifier head on a ragged batch: what token paddings cost, and what they save.

B = 32 clips of S = 4096 tokens, D = 768, 12 heads, 400 classes, bf16 tokens, forward + backward in one process
(vp_op_probe_forward + vp_op_probe_backward, and their *_masked forms):

  (a) unmasked                       the call without paddings
  (b) masked, nothing padded         the same work through the masked kernels: the cost of carrying the mask
  (c) masked, half the tokens padded suffix lengths drawn once from a fixed seed, scaled so that exactly half of the
                                     B * S tokens are padded
  (d) unmasked at S / 2              a batch of half the tokens: what (c) would cost if padding were free

Each is timed with HIP events over `--iters` calls per round; the variants alternate round by round; median, minimum
and maximum over `--rounds` rounds.  Reported, not barred: (b) / (a) and (c) / (d).  The forwards of (a), (c) and (d)
are also timed alone (the backward is the difference), to show where the time of a half-padded batch goes.

    python tools/probe_ragged_bench.py [--out profiles/probe_masked/bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import torch  # noqa: E402

from videoprism import _native  # noqa: E402
from videoprism.probe import AttentiveProbe  # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def half_padded_lengths(B, S, seed):
    """B valid lengths in [1, S], drawn once from `seed`, that sum to exactly B * S / 2."""
    g = torch.Generator().manual_seed(seed)
    n = (torch.rand(B, generator=g) * S).long().clamp(1, S)
    want = B * S // 2
    n = (n.double() * want / n.sum().item()).long().clamp(1, S)
    i = 0
    while n.sum().item() != want:  # the rounding's remainder, one token at a time
        step = 1 if n.sum().item() < want else -1
        if 1 <= n[i % B].item() + step <= S:
            n[i % B] += step
        i += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--classes", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_ragged_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    B, S, D, H, C = args.clips, args.tokens, args.dim, args.heads, args.classes
    dims = (D, H, C)
    g = torch.Generator(device=dev).manual_seed(0)
    tokens = torch.randn((B, S, D), generator=g, device=dev).to(torch.bfloat16)
    short = tokens[:, :S // 2].contiguous()
    dlogits = torch.randn((B, C), generator=g, device=dev)
    probe = AttentiveProbe(D, H, C, device=dev, seed=0)
    tensors = {m: probe.get_parameter(path).detach() for m, path in _native.PROBE_LEAVES}
    grads = {m: torch.empty_like(t) for m, t in tensors.items()}
    ws = torch.empty(_native.op_probe_workspace_bytes(*dims, B, S), dtype=torch.uint8, device=dev)
    logits = torch.empty((B, C), device=dev)
    lengths = half_padded_lengths(B, S, args.seed)
    none = torch.zeros((B, S), device=dev)
    half = (torch.arange(S)[None, :] >= lengths[:, None]).float().to(dev)
    assert int(half.sum().item()) == B * S // 2

    def forward(x, pad):
        _native.op_probe_forward(dims, tensors, x, logits, None, ws, paddings=pad)

    def both(x, pad):
        forward(x, pad)
        _native.op_probe_backward(dims, tensors, x, dlogits, grads, ws, paddings=pad)

    variants = {"(a) unmasked": lambda: both(tokens, None),
                "(b) masked, none padded": lambda: both(tokens, none),
                "(c) masked, half padded": lambda: both(tokens, half),
                "(d) unmasked, S / 2": lambda: both(short, None),
                "(a) forward alone": lambda: forward(tokens, None),
                "(c) forward alone": lambda: forward(tokens, half),
                "(d) forward alone": lambda: forward(short, None)}
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):  # alternating rounds
        for k, fn in variants.items():
            times[k].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in times.items()}

    lines = [f"probe_ragged_bench: {torch.cuda.get_device_name(0)}; B={B} S={S} D={D} heads={H} classes={C} bf16 tokens; "
             f"forward + backward unless said; {args.rounds} rounds x {args.iters} calls (HIP events), variants alternating",
             f"  (c): suffix paddings, valid lengths from seed {args.seed}: min {int(lengths.min())}, max "
             f"{int(lengths.max())}, {int(half.sum().item())} of {B * S} tokens padded"]
    for k, v in times.items():
        lines.append(f"  {k:26s} median {med[k]:8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}")
    a, b, c, d = (med[k] for k in list(variants)[:4])
    lines.append(f"  (b) / (a) = {b / a:.3f}: the cost of carrying the mask")
    lines.append(f"  (c) / (d) = {c / d:.3f}: a half-padded batch against a batch of half the tokens; (c) / (a) = {c / a:.3f}")
    fa, fc, fd = med["(a) forward alone"], med["(c) forward alone"], med["(d) forward alone"]
    lines.append(f"  forward alone: (c) / (d) = {fc / fd:.3f}, (c) / (a) = {fc / fa:.3f}; backward (difference): "
                 f"(c) {c - fc:.4f} ms, (d) {d - fd:.4f} ms, (a) {a - fa:.4f} ms")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
