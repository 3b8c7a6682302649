"""Searching a gallery of a million embeddings stored as fp8 (e4m3 codes and a power-of-two scale per row) against
the same gallery stored as bf16, and what the smaller format costs in accuracy.

N = 1,000,000 unit rows, D = 768 and 1024, Q = 1, 32 and 256 queries, k = 10, in one process.  The fp8 and the bf16
index alternate round by round, each timed with HIP events over `--iters` calls of EmbeddingIndex.search per round,
median over `--rounds` rounds, spread = (max - min) / median.  The ratio fp8 / bf16 is set against the spread the bf16
rounds show among themselves: fp8 counts as slower only where it is slower by more than that.  Each search is also set
against the bytes it has to read (the gallery once per group of queries, fp8: D + 4 bytes a row) as a share of the
6.3 TB/s measured copy rate.

Accuracy, on these synthetic rows (unit-norm Gaussian, unstructured: the hard case for recall, not a model's
embeddings), for the Q = 256 queries against an fp32 index of the same rows: the error of the returned scores against
the fp64 score of the same row of the unrounded gallery (max and rms), and recall@10 = the share of the fp32 index's
10 ids that the smaller index returns.

    python tools/retrieval_f8_bench.py [--out profiles/retrieval_f8/retrieval_f8_bench.txt]
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

COPY_RATE = 6.3e12  # bytes/s, measured device copy rate on MI355X


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def accuracy(index, exact_index, base, q, k):
    """(max, rms) of |returned score - fp64 score of that row of `base`| and recall@k against exact_index."""
    s, i = index.search(q, k)
    _, want = exact_index.search(q, k)
    ref = torch.einsum("qkd,qd->qk", base[i].double(), q.double())
    err = (s.double() - ref).abs()
    hit = (i[:, :, None] == want[:, None, :]).any(dim=2).float().mean()
    return float(err.max()), float(err.pow(2).mean().sqrt()), float(hit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_f8_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    N, k = args.rows, args.k
    lines = [f"retrieval_f8_bench: {torch.cuda.get_device_name(0)}; N={N} k={k}; fp8 and bf16 index alternating, median "
             f"of {args.rounds} rounds of {args.iters} searches (HIP events); spread = (max - min) / median"]
    slower = []
    for D in args.dims:
        gen = torch.Generator(device=dev).manual_seed(D)
        base = torch.nn.functional.normalize(torch.randn((N, D), generator=gen, device=dev), dim=1)
        f8 = EmbeddingIndex(D, dtype=torch.float8_e4m3fn, device=dev, capacity=N)
        bf = EmbeddingIndex(D, dtype=torch.bfloat16, device=dev, capacity=N)
        f8.add(base)
        bf.add(base)
        row_f8, row_bf = D + 4, 2 * D
        lines.append(f"  D={D}: {row_f8} B a row against {row_bf} B ({row_bf / row_f8:.2f}x the rows in the same memory)")
        for Q in args.queries:
            q = torch.nn.functional.normalize(torch.randn((Q, D), generator=gen, device=dev), dim=1)
            for _ in range(args.warmup):
                f8.search(q, k)
                bf.search(q, k)
            torch.cuda.synchronize()
            t8, tb = [], []
            for _ in range(args.rounds):
                t8.append(timed(lambda: f8.search(q, k), args.iters))
                tb.append(timed(lambda: bf.search(q, k), args.iters))
            m8, mb = statistics.median(t8), statistics.median(tb)
            s8, sb = (max(t8) - min(t8)) / m8, (max(tb) - min(tb)) / mb
            G = _native.load().vp_dev_topk_group(D, k)
            groups = (Q + G - 1) // G
            r8, rb = N * row_f8 * groups / (m8 * 1e-3), N * row_bf * groups / (mb * 1e-3)
            verdict = "slower than bf16 beyond its spread" if m8 > mb * (1 + sb) else "not slower"
            if m8 > mb * (1 + sb):
                slower.append(f"D={D} Q={Q}")
            lines.append(
                f"  D={D:4d} Q={Q:3d}: fp8 {m8:7.3f} ms (spread {s8:.1%}) | bf16 {mb:7.3f} ms (spread {sb:.1%}) | fp8 / bf16 "
                f"{m8 / mb:.3f}: {verdict} | {groups} group(s) of {G}: fp8 {r8 / 1e12:5.2f} TB/s = {r8 / COPY_RATE:.1%} of the "
                f"copy rate, bf16 {rb / 1e12:5.2f} TB/s = {rb / COPY_RATE:.1%}")
        exact = EmbeddingIndex(D, dtype=torch.float32, device=dev, capacity=N)
        exact.add(base)
        for name, index in (("fp8", f8), ("bf16", bf)):
            emax, erms, recall = accuracy(index, exact, base, q, k)
            lines.append(f"  D={D:4d} {name:4s} against the fp32 index, Q={q.shape[0]} (synthetic unit rows): score error max "
                         f"{emax:.2e} rms {erms:.2e}, recall@{k} {recall:.3f}")
        del f8, bf, exact, base
    lines.append("  finding: fp8 slower than bf16 beyond the bf16 spread at " + ", ".join(slower) if slower else
                 "  fp8 not slower than bf16 at any shape")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
