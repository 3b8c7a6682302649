"""Searching a gallery of a million embeddings: EmbeddingIndex.search against the route the library offered before it.

N = 1,000,000 unit rows, D = 768 and 1024, Q = 1, 32 and 256 queries, k = 10, fp32 and bf16 gallery, in one process.
The two routes alternate round by round, each timed with HIP events over `--iters` calls per round, median over
`--rounds` rounds, spread = (max - min) / median:

  search   EmbeddingIndex.search (vp_op_topk: per-range candidate lists, then their merge)
  parent   _native.op_similarity (one workgroup per (row, query) pair, an [N, Q] fp32 matrix) followed by torch.topk
           over the rows.  op_similarity takes fp32 only, so it reads an fp32 copy of the stored gallery made outside
           the timed region.  From Q = 32 on it is timed over the first `--parent-rows` rows (it launches N * Q
           workgroups); the line says so and scales the time by N / rows.

Each search is set against the bytes it has to read, the gallery once per group of queries (32, or 16 where the
kernel's group is 16), as a share of the 6.3 TB/s measured copy rate, and against the time its MFMAs need at the spec
rate (fp32 157.3 TFLOP/s; bf16 2.5 PFLOP/s, two products per element for the split query; always 32 query columns
per group), and the larger of the two floors is named as the bound.

    python tools/retrieval_bench.py [--out profiles/retrieval/retrieval_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import torch  # noqa: E402

from videoprism import _native  # noqa: E402
from videoprism.retrieval import EmbeddingIndex  # noqa: E402

COPY_RATE = 6.3e12                                  # bytes/s, measured device copy rate on MI355X
MFMA_RATE = {"fp32": 157.3e12, "bf16": 2.5e15}      # FLOP/s, spec


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--parent-rows", type=int, default=100_000, help="rows the parent's route is timed over from Q = 32 on")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent-iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    N, k = args.rows, args.k
    lines = [f"retrieval_bench: {torch.cuda.get_device_name(0)}; N={N} k={k}; median of {args.rounds} alternating rounds "
             f"(search x {args.iters}, parent x {args.parent_iters} calls, HIP events); spread = (max - min) / median"]
    slower = []
    for D in args.dims:
        gen = torch.Generator(device=dev).manual_seed(D)
        base = torch.nn.functional.normalize(torch.randn((N, D), generator=gen, device=dev), dim=1)
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            index = EmbeddingIndex(D, dtype=dtype, device=dev, capacity=N)
            index.add(base)
            g32 = index.embeddings.float() if dtype != torch.float32 else index.embeddings  # the parent's operand
            for Q in args.queries:
                q = torch.nn.functional.normalize(torch.randn((Q, D), generator=gen, device=dev), dim=1)
                n_par = N if Q < 32 else min(N, args.parent_rows)

                def search():
                    return index.search(q, k)

                def parent():
                    return torch.topk(_native.op_similarity(g32[:n_par], q), k, dim=0)

                for _ in range(args.warmup):
                    search()
                    parent()
                torch.cuda.synchronize()
                ts, tp = [], []
                for _ in range(args.rounds):
                    ts.append(timed(search, args.iters))
                    tp.append(timed(parent, args.parent_iters))
                ms, mp = statistics.median(ts), statistics.median(tp) * (N / n_par)
                ss, sp = (max(ts) - min(ts)) / ms, (max(tp) - min(tp)) / statistics.median(tp)
                G = _native.load().vp_dev_topk_group(D, k)
                groups = (Q + G - 1) // G
                nbytes = N * D * index.embeddings.element_size() * groups
                flops = 2.0 * N * D * 32 * groups * (2 if name == "bf16" else 1)
                t_mem, t_mfma = nbytes / COPY_RATE * 1e3, flops / MFMA_RATE[name] * 1e3
                rate = nbytes / (ms * 1e-3)
                bound = "bandwidth" if t_mem >= t_mfma else "MFMA rate"
                scaled = "" if n_par == N else f" (timed over {n_par} rows, x{N / n_par:g})"
                lines.append(
                    f"  D={D:4d} {name} Q={Q:3d}: search {ms:8.3f} ms (spread {ss:.1%}) | parent {mp:9.3f} ms (spread {sp:.1%})"
                    f"{scaled} | x{mp / ms:7.1f} | {groups} group(s) of {G}: {nbytes / 1e9:6.2f} GB -> {rate / 1e12:5.2f} TB/s = "
                    f"{rate / COPY_RATE:.1%} of the copy rate | floors: memory {t_mem:.3f} ms, MFMA {t_mfma:.3f} ms: bound by {bound}")
                if ms * (1 - ss) > mp:
                    slower.append(f"D={D} {name} Q={Q}")
            del index, g32
        del base
    lines.append("  finding: search slower than the parent's route at " + ", ".join(slower) if slower else
                 "  search faster than the parent's route at every shape")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
