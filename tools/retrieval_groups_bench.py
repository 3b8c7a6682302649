"""The k best videos of a gallery of windows: EmbeddingIndex.search_groups against the ungrouped search of the same
gallery (the floor: it reads the same rows once) and against the route there was before it, over-fetching rows and
deduplicating them.

N = 1,000,000 unit rows, D = 768, bf16 gallery, k = 10, Q = 1, 32 and 256 queries, in one process.  The gallery is
N / 64 videos of 64 windows each, a video's windows drawn around a common direction (`--sigma` sets how far) so that
they score alike.  Labelings:

  a  row // 64: a video's windows are neighbours.  The case the feature is for, and the one where candidates of a
     group that is in the list already (they change nothing, or replace in place) are most frequent
  b  the same labels randomly permuted over the rows: a group's rows are unrelated
  c  every row its own group (not a use case: it has the label reads and the wider lists but no same-group candidate,
     so a - c is what those candidates cost)

Routes, alternating round by round, each timed with HIP events over `--iters` calls per round; median over `--rounds`
rounds, spread = (max - min) / median:

  groups    index.search_groups(q, 10)
  search    index.search(q, 10)
  overfetch index.search(q, 128), the kernel's maximum, then in torch on the device: the labels of the 128 rows, the
            first row of every label, the first 10 of those.  Its result is also compared with `groups`: the share of
            queries where it finds fewer than 10 distinct videos, and where it differs at all.

    python tools/retrieval_groups_bench.py [--out profiles/retrieval_groups/bench.txt]
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

PER_VIDEO = 64
FETCH = 128


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def dedup(scores, ids, labels, k):
    """Rows [Q, FETCH] in search's order -> the first row of every label, the first k of those: (scores, groups, ids)
    padded with (-inf, -1, -1)."""
    lab = torch.where(ids >= 0, labels[ids.clamp(min=0)], torch.full_like(ids, -1))
    same = lab[:, :, None] == lab[:, None, :]
    first = ~torch.tril(same, diagonal=-1).any(dim=2) & (lab >= 0)
    pos = torch.arange(lab.shape[1], device=lab.device)
    key = torch.where(first, pos, pos + lab.shape[1])
    at = torch.topk(key, k, dim=1, largest=False).indices  # the first k firsts, in order
    ok = torch.gather(first, 1, at)
    neg = torch.full_like(at, -1)
    return (torch.where(ok, torch.gather(scores, 1, at), torch.full_like(at, float("-inf"), dtype=scores.dtype)),
            torch.where(ok, torch.gather(lab, 1, at), neg), torch.where(ok, torch.gather(ids, 1, at), neg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.2, help="length of a window's own part against its video's unit direction")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_groups_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    N, D, k = args.rows, args.dim, args.k
    videos = (N + PER_VIDEO - 1) // PER_VIDEO
    gen = torch.Generator(device=dev).manual_seed(D)
    norm = torch.nn.functional.normalize
    centre = norm(torch.randn((videos, D), generator=gen, device=dev), dim=1)
    base = norm(centre.repeat_interleave(PER_VIDEO, dim=0)[:N]
                + args.sigma * norm(torch.randn((N, D), generator=gen, device=dev), dim=1), dim=1)
    by_video = torch.arange(N, device=dev) // PER_VIDEO
    labelings = (("a row // 64", by_video), ("b permuted", by_video[torch.randperm(N, generator=gen, device=dev)]),
                 ("c own group", torch.arange(N, device=dev)))
    lib = _native.load()
    lines = [f"retrieval_groups_bench: {torch.cuda.get_device_name(0)}; N={N} D={D} bf16 k={k}; {videos} videos of "
             f"{PER_VIDEO} windows, sigma {args.sigma:g}; median of {args.rounds} alternating rounds x {args.iters} calls "
             f"(HIP events); spread = (max - min) / median; queries per workgroup: groups "
             f"{lib.vp_dev_topk_groups_group(D, k)}, search k={k} {lib.vp_dev_topk_group(D, k)}, "
             f"search k={FETCH} {lib.vp_dev_topk_group(D, FETCH)}"]
    for name, labels in labelings:
        index = EmbeddingIndex(D, dtype=torch.bfloat16, device=dev, capacity=N)
        index.add(base, group=labels)
        for Q in args.queries:
            q = norm(torch.randn((Q, D), generator=torch.Generator(device=dev).manual_seed(Q), device=dev), dim=1)
            routes = {"groups": lambda: index.search_groups(q, k), "search": lambda: index.search(q, k),
                      "overfetch": lambda: dedup(*index.search(q, FETCH), labels, k)}
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            t = {r: [] for r in routes}
            for _ in range(args.rounds):
                for r, fn in routes.items():
                    t[r].append(timed(fn, args.iters))
            med = {r: statistics.median(v) for r, v in t.items()}
            spread = {r: (max(v) - min(v)) / med[r] for r, v in t.items()}
            want, got = routes["groups"](), routes["overfetch"]()
            torch.cuda.synchronize()
            short = (got[1] < 0).any(dim=1)
            differs = short | (got[1] != want[1]).any(dim=1) | (got[2] != want[2]).any(dim=1)
            lines.append(
                f"  {name:11s} Q={Q:3d}: groups {med['groups']:7.3f} ms (spread {spread['groups']:.1%}) | search "
                f"{med['search']:7.3f} ms (spread {spread['search']:.1%}) | groups / search x{med['groups'] / med['search']:.2f}"
                f" | overfetch {med['overfetch']:7.3f} ms (spread {spread['overfetch']:.1%}), x{med['overfetch'] / med['groups']:.2f}"
                f" of groups; fewer than {k} videos for {short.float().mean().item():.1%} of the queries, differs for "
                f"{differs.float().mean().item():.1%}")
        del index
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
