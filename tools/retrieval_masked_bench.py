"""Searching a subset of a gallery of a million embeddings: the masked search against the unmasked one and against
gathering the allowed rows first.

N = 1,000,000 unit rows, D = 768 and 1024, Q = 1, 32 and 256 queries, k = 10, fp32 and bf16 gallery, in one process.
One mask for all queries, at allowed fractions 1.0, 0.5, 0.1 and 0.01, laid out two ways:

  random   every row allowed with that probability: nearly every wave of 64 rows holds an allowed row, so nothing is
           skipped but the loads of the rows that are not allowed
  blocked  whole blocks of `--block` rows (4096) allowed or not: the waves inside a block that is not allowed skip
           their loads and MFMAs, which is where the masked scan should approach the cost of its allowed rows

The arms alternate round by round, each timed with HIP events over `--iters` calls per round, median over `--rounds`
rounds, spread = (max - min) / median:

  unmasked  _native.op_topk on the whole gallery (the kernel the masked scan must stay close to at fraction 1.0)
  parent    the same call through another build's library (`--parent LIB.so`, tools/ab_build.sh): the unmasked search
            of the revision before the masked one, on the same box in the same session
  masked    _native.op_topk_masked with the packed mask (packed outside the timed region; the pack kernel is timed on
            its own line)
  gather    the alternative a caller has without the mask: gallery[rows] into a second gallery, then op_topk on it
            (the row numbers are made outside the timed region; the ids would still need mapping back)

`rows` is the unmasked time scaled by the allowed fraction: what the allowed rows alone would cost at the unmasked
rate, the figure the blocked masks are set against.  Every masked result is compared with the gathered one, ids
mapped back, bit for bit, at the size timed.

    python tools/retrieval_masked_bench.py [--parent LIB.so] [--out profiles/retrieval_masked/retrieval_masked_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import torch  # noqa: E402

from videoprism import _native  # noqa: E402

FRACTIONS = (1.0, 0.5, 0.1, 0.01)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def make_allow(N, fraction, layout, block, gen):
    """bool [N] on the device: rows allowed with probability `fraction`, one by one or in whole blocks."""
    if fraction >= 1.0:
        return torch.ones(N, dtype=torch.bool, device=gen.device)
    if layout == "random":
        return torch.rand(N, generator=gen, device=gen.device) < fraction
    nb = (N + block - 1) // block
    on = torch.rand(nb, generator=gen, device=gen.device) < fraction
    return on.repeat_interleave(block)[:N]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--block", type=int, default=4096, help="rows of a block of the blocked masks")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="another build's libvideoprism_hip.so: its vp_op_topk is timed too")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_masked_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    N, k = args.rows, args.k
    parent = None
    if args.parent:
        parent = ctypes.CDLL(args.parent).vp_op_topk
        parent.restype, parent.argtypes = _native._SIGNATURES["vp_op_topk"]
    lines = [f"retrieval_masked_bench: {torch.cuda.get_device_name(0)}; N={N} k={k}; one mask for all queries; blocks of "
             f"{args.block} rows; median of {args.rounds} alternating rounds x {args.iters} calls (HIP events); spread = "
             f"(max - min) / median; parent = {args.parent or 'not given'}"]
    findings = []
    for D in args.dims:
        gen = torch.Generator(device=dev).manual_seed(D)
        base = torch.nn.functional.normalize(torch.randn((N, D), generator=gen, device=dev), dim=1)
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            g = base.to(dtype)
            masks = {}
            for layout in ("random", "blocked"):
                for f in FRACTIONS:
                    if f >= 1.0 and layout == "blocked":
                        continue
                    allow = make_allow(N, f, layout, args.block, gen)
                    masks[(layout, f)] = (allow, _native.op_rowmask_pack(allow), allow.nonzero().reshape(-1))
            allow = masks[("random", 0.5)][0]
            t_pack = statistics.median(timed(lambda: _native.op_rowmask_pack(allow), args.iters)
                                       for _ in range(args.rounds))
            lines.append(f"  D={D:4d} {name}: vp_op_rowmask_pack of {N} rows {t_pack * 1e3:7.1f} us")
            for Q in args.queries:
                q = torch.nn.functional.normalize(torch.randn((Q, D), generator=gen, device=dev), dim=1)
                ws = torch.empty(_native.op_topk_workspace_bytes(Q, k), dtype=torch.uint8, device=dev)
                ps, pi = torch.empty((Q, k), device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev)

                def run_parent():
                    rc = parent(_native._ptr(q), Q, _native._ptr(g), _native._prec(g), N, D, D, k, 0, _native._ptr(ps),
                                _native._ptr(pi), _native._ptr(ws), ws.numel(), _native._stream())
                    assert rc == 0, rc

                arms = {"unmasked": lambda: _native.op_topk(q, g, k, ws=ws)}
                if parent is not None:
                    arms["parent"] = run_parent
                for (layout, f), (_, words, rows) in masks.items():
                    arms[f"masked {layout} {f:g}"] = lambda words=words: _native.op_topk_masked(q, g, k, words, ws=ws)
                    if layout == "random" and f < 1.0:
                        arms[f"gather {f:g}"] = lambda rows=rows: _native.op_topk(q, g[rows], k, ws=ws)
                # the results, before anything is timed: masked == gathered with the ids mapped back, bit for bit
                same = True
                for (layout, f), (_, words, rows) in masks.items():
                    ms_, mi_ = _native.op_topk_masked(q, g, k, words, ws=ws)
                    gs_, gi_ = _native.op_topk(q, g[rows], k)
                    gi_ = torch.where(gi_ >= 0, rows[gi_.clamp(min=0)], gi_)
                    same &= bool(torch.equal(ms_.view(torch.int32), gs_.view(torch.int32)) and torch.equal(mi_, gi_))
                if parent is not None:
                    us, ui = _native.op_topk(q, g, k, ws=ws)
                    run_parent()
                    same &= bool(torch.equal(us.view(torch.int32), ps.view(torch.int32)) and torch.equal(ui, pi))
                for _ in range(args.warmup):
                    for fn in arms.values():
                        fn()
                torch.cuda.synchronize()
                t = {a: [] for a in arms}
                for _ in range(args.rounds):
                    for a, fn in arms.items():
                        t[a].append(timed(fn, args.iters))
                med = {a: statistics.median(v) for a, v in t.items()}
                spread = {a: (max(v) - min(v)) / med[a] for a, v in t.items()}
                un = med["unmasked"]
                lines.append(f"  D={D:4d} {name} Q={Q:3d}: results bitwise equal: {same} | unmasked {un:7.3f} ms (spread "
                             f"{spread['unmasked']:.1%})" + (f" | parent {med['parent']:7.3f} ms (spread "
                                                             f"{spread['parent']:.1%})" if parent is not None else ""))
                for a in arms:
                    if a in ("unmasked", "parent"):
                        continue
                    f = float(a.split()[-1])
                    lines.append(f"      {a:20s} {med[a]:7.3f} ms (spread {spread[a]:.1%}) = x{med[a] / un:5.2f} of unmasked"
                                 f" | rows {un * f:7.3f} ms")
                ones = med["masked random 1"]
                noise = max(spread["unmasked"], spread["masked random 1"]) * un
                if ones - un > noise:
                    findings.append(f"D={D} {name} Q={Q}: all-ones mask {ones - un:+.3f} ms = {ones / un - 1:+.1%} over "
                                    f"the unmasked search, outside the spread ({noise:.3f} ms)")
                if not same:
                    findings.append(f"D={D} {name} Q={Q}: RESULTS DIFFER")
            del g, masks
        del base
    lines.append("  finding: " + "; ".join(findings) if findings else
                 "  the all-ones mask is within the spread of the unmasked search at every shape; all results bitwise equal")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
