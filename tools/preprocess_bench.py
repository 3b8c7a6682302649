"""Frame preprocessing (csrc/preprocess.hip) beside the forward it feeds, at the bench step: 512 frames
(B = 32 clips x T = 16) from 360 x 640 and 720 x 1280 uint8 sources already on the device, centre
crop to 288.  Prints frames/s and effective GB/s of the launch (HIP events after warm-up; bytes = the
part of every touched source row between the first and last tap, plus the bytes written) and, from the
same process, the Base bf16 vp_forward time of the step on 288 x 288 uint8 frames.  The condition the
kernel is held to: preprocessing adds no more than 10 % to the forward step.

    python tools/preprocess_bench.py [--out profiles/preprocess_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from videoprism import models, params, video_utils  # noqa: E402


def timeit(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def tap_span(dst, src, lo, n):
    """First and last source index the outputs lo .. lo+n-1 of a `dst`-long axis read (cv2's table)."""
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(lo, lo + n) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.clip(np.floor(f).astype(np.int64), 0, src - 1)
    return int(s.min()), int(min(s.max() + 1, src - 1))


def touched_bytes(h, w, size):
    new_h, new_w, y0, x0 = video_utils.center_crop_geometry(h, w, size)
    ya, yb = tap_span(new_h, h, y0, size)
    xa, xb = tap_span(new_w, w, x0, size)
    return (yb - ya + 1) * (xb - xa + 1) * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    B, T, S = args.batch, args.frames, 288
    F = B * T

    name = "videoprism_public_v1_base"
    model = models.get_model(name, fprop_dtype=torch.bfloat16)
    cfg = dict(models.CONFIGS["videoprism_v1_base"])
    eng = model.engine(params.synthetic_params(cfg, seed=0), 0)
    out = torch.empty((B, T * 256, cfg["model_dim"]), dtype=torch.bfloat16, device=dev)

    g = torch.Generator(device=dev).manual_seed(0)
    fns, nbytes = {}, {}
    frames = None
    for h, w in ((360, 640), (720, 1280)):
        src = torch.randint(0, 256, (B, T, h, w, 3), generator=g, device=dev, dtype=torch.uint8)
        key = f"preprocess_{h}x{w}"
        fns[key] = lambda src=src: video_utils.preprocess_frames(src)
        nbytes[key] = F * (touched_bytes(h, w, S) + S * S * 3)
        frames = fns[key]()
    fns["vp_forward"] = lambda: eng.forward(frames, out=out)

    res = {k: [] for k in fns}
    for _ in range(args.rounds):  # interleaved, so a drift of the machine falls on every row alike
        for k, f in fns.items():
            res[k].append(timeit(f, iters=3 if k == "vp_forward" else 20, warm=2))
    fwd = statistics.median(res["vp_forward"])
    rec = {"tool": "preprocess_bench", "device": torch.cuda.get_device_name(0), "batch": B, "frames_per_clip": T,
           "target_size": S, "rounds": args.rounds,
           "vp_forward": {"model": name, "dtype": "bf16", "input": "uint8 288x288", "ms_median": round(fwd, 4),
                          "ms_min": round(min(res["vp_forward"]), 4), "clips_per_s": round(B / fwd * 1e3, 1)}}
    ok = True
    for k in fns:
        if k == "vp_forward":
            continue
        ms = statistics.median(res[k])
        rec[k] = {"ms_median": round(ms, 4), "ms_min": round(min(res[k]), 4), "ms_max": round(max(res[k]), 4),
                  "frames_per_s": round(F / ms * 1e3), "bytes": nbytes[k], "effective_GB_per_s": round(nbytes[k] / ms / 1e6, 1),
                  "share_of_forward": round(ms / fwd, 4)}
        ok = ok and ms <= 0.10 * fwd
        print(f"{k}: {ms:.3f} ms (min {min(res[k]):.3f}) = {F / ms * 1e3:,.0f} frames/s, {nbytes[k] / ms / 1e6:,.0f} GB/s "
              f"effective over {nbytes[k] / 1e6:.0f} MB; {100 * ms / fwd:.2f} % of the forward step", flush=True)
    print(f"vp_forward ({name}, bf16, uint8 frames): {fwd:.2f} ms = {B / fwd * 1e3:,.0f} clips/s", flush=True)
    rec["within_10_percent_of_forward"] = ok
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
