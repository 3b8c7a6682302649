"""Training the classifier head on frozen tokens: what a step costs at Base's shape.

B = 32 clips of S = 4096 tokens (16 frames x 256 patches), D = 768, 12 heads, 400 classes, bf16 tokens, in one
process: the head's forward (vp_op_probe_forward), forward plus backward, and each of the backward's two streaming
passes alone (pass 1: dl from the tokens; pass 2: dU with its reduction).  Each is timed with HIP events over
`--iters` calls per round, median over `--rounds` rounds; the variants alternate round by round.

Each pass is set against its algorithmic traffic (bytes computed from the shapes, below) as achieved bytes/s and as
a share of the 8 TB/s HBM peak; forward and forward + backward against the four token reads they make plus the
same side traffic.  Expectation from the code: the backward costs about what the forward does (two passes each);
backward / forward above 2 in this run is reported as a finding.

    python tools/probe_bench.py [--out profiles/probe/probe_bench.txt]
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

PEAK_HBM = 8.0e12  # bytes/s, MI355X HBM3E (spec)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def traffic(B, S, D, H, es):
    """Algorithmic bytes of each streaming pass: the tokens once, plus the per-(clip, head, token) fp32 rows it reads
    and writes and, for the weighted sums, the chunk partials written and read back by the reduction."""
    tok, row = B * S * D * es, B * H * S * 4
    part = B * _native.dev_pool_chunks(S) * H * D * 4
    return {"fwd_logits": tok + row, "fwd_wsum": tok + 2 * row + 2 * part,  # the statistics read the logits too
            "pass1": tok + 2 * row, "pass2": tok + row + 2 * part}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--classes", type=int, default=400)
    ap.add_argument("--fp32", action="store_true", help="fp32 tokens instead of bf16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    B, S, D, H, C = args.clips, args.tokens, args.dim, args.heads, args.classes
    dims = (D, H, C)
    g = torch.Generator(device=dev).manual_seed(0)
    tokens = torch.randn((B, S, D), generator=g, device=dev).to(torch.float32 if args.fp32 else torch.bfloat16)
    dlogits = torch.randn((B, C), generator=g, device=dev)
    probe = AttentiveProbe(D, H, C, device=dev, seed=0)
    tensors = {m: probe.get_parameter(path).detach() for m, path in _native.PROBE_LEAVES}
    grads = {m: torch.empty_like(t) for m, t in tensors.items()}
    ws = torch.empty(_native.op_probe_workspace_bytes(*dims, B, S), dtype=torch.uint8, device=dev)
    logits = torch.empty((B, C), device=dev)

    def forward():
        _native.op_probe_forward(dims, tensors, tokens, logits, None, ws)

    def both():
        forward()
        _native.op_probe_backward(dims, tensors, tokens, dlogits, grads, ws)

    variants = {"forward": forward, "forward+backward": both,
                "pass1": lambda: _native.dev_probe_backward_pass(dims, tokens, 1, ws),
                "pass2": lambda: _native.dev_probe_backward_pass(dims, tokens, 2, ws)}
    both()  # the passes run on a workspace the backward has filled
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):  # alternating rounds
        for k, fn in variants.items():
            times[k].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}

    es = tokens.element_size()
    t = traffic(B, S, D, H, es)
    fwd_bytes = t["fwd_logits"] + t["fwd_wsum"]
    both_bytes = fwd_bytes + t["pass1"] + t["pass2"]
    nbytes = {"forward": fwd_bytes, "forward+backward": both_bytes, "pass1": t["pass1"], "pass2": t["pass2"]}
    backward = med["forward+backward"] - med["forward"]
    ratio = backward / med["forward"]
    lines = [f"probe_bench: {torch.cuda.get_device_name(0)}; B={B} S={S} D={D} heads={H} classes={C} "
             f"{'fp32' if args.fp32 else 'bf16'} tokens; median of {args.rounds} rounds x {args.iters} calls (HIP events)"]
    for k in variants:
        rate = nbytes[k] / (med[k] * 1e-3)
        lines.append(f"  {k:17s} {med[k]:8.4f} ms  (spread {spread[k]:.1%})  algorithmic traffic {nbytes[k] / 1e6:8.1f} MB"
                     f"  -> {rate / 1e12:5.2f} TB/s = {rate / PEAK_HBM:.1%} of the HBM peak")
    small = backward - med["pass1"] - med["pass2"]
    lines.append(f"  backward (difference) {backward:.4f} ms = {ratio:.2f} x forward; outside the two passes "
                 f"{small:.4f} ms (the parameter-sized kernels)")
    lines.append(f"  finding: backward / forward = {ratio:.2f} > 2" if ratio > 2.0 else
                 f"  backward / forward = {ratio:.2f}: within the expected 2")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
