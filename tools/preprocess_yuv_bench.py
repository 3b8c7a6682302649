"""Frame ingest from a decoder's 4:2:0 planes (preprocess_yuv_kernel, csrc/preprocess.hip) beside the packed-RGB
kernel on frames of the same resolution: 16-frame clips at 1280 x 720 and 1920 x 1080, centre crop to 288, the
sources already on the device.  One launch preprocesses one clip.  Per resolution and format the launches are
timed in windows (HIP events around `--iters` launches, each on another clip of a pool too large for the
256 MiB Infinity Cache, so the planes come from HBM as they would behind a decoder); a YUV window alternates
with an RGB window, `--rounds` times, and the record keeps the median, the minimum and the maximum window of
both.  Before timing, one frame per format and resolution is compared bitwise with the RGB kernel run on the
converted frame (tests/yuv_restatement.py).

The condition the NV12 kernel is held to: no slower than 1.10 x the RGB kernel on the same shapes in the same
session.  I420 and P010 are recorded without a condition.

    python tools/preprocess_yuv_bench.py [--format nv12 i420 p010] [--out profiles/yuv_ingest/bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yuv_restatement as yr  # noqa: E402
from videoprism import _native as nat  # noqa: E402
from videoprism import video_utils  # noqa: E402

SIZES = ((720, 1280), (1080, 1920))
T, S = 16, 288
FORMATS = {"nv12": nat.VP_YUV_NV12, "i420": nat.VP_YUV_I420, "p010": nat.VP_YUV_P010}
MATRICES = {"bt601": nat.VP_YUV_BT601, "bt709": nat.VP_YUV_BT709}


def source_bytes(fmt, h, w):
    """Bytes of one frame's planes."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return {"rgb": 3 * h * w, "nv12": h * w + 2 * ch * cw, "i420": h * w + 2 * ch * cw,
            "p010": 2 * (h * w + 2 * ch * cw)}[fmt]


def make_pool(fmt, h, w, clips, gen, dev):
    """`clips` clips of T random frames on the device, as the tuple of planes (or the RGB tensor) of each."""
    ch, cw = (h + 1) // 2, (w + 1) // 2

    def rand(*shape):
        if fmt == "p010":  # every bit random: the low 6 are ignored
            return (torch.randint(0, 65536, shape, generator=gen, device=dev, dtype=torch.int32) - 32768).to(torch.int16)
        return torch.randint(0, 256, shape, generator=gen, device=dev, dtype=torch.uint8)

    pool = []
    for _ in range(clips):
        if fmt == "rgb":
            pool.append(rand(T, h, w, 3))
        elif fmt == "i420":
            pool.append((rand(T, h, w), rand(T, ch, cw), rand(T, ch, cw)))
        else:
            pool.append((rand(T, h, w), rand(T, ch, cw, 2)))
    return pool


def launcher(fmt, pool, h, w, out):
    """A function that preprocesses the pool's next clip into `out`.  It calls the C entry point with arguments
    built once, so a window measures the kernel and not Python: the wrappers' checks take longer than a launch."""
    lib = nat.load()
    stream = nat._stream()
    matrix = MATRICES[video_utils.yuv_matrix("auto", h, w)]
    calls = []
    for src in pool:
        if fmt == "rgb":
            calls.append((lib.vp_op_preprocess_frames, (nat._ptr(src), T, h, w, src.stride(1), src.stride(0), None, T,
                                                        nat.VP_RESIZE_CENTER_CROP, 0, S, nat._ptr(out), stream)))
        else:
            frames, n, _, _ = nat.yuv_frames(src, FORMATS[fmt], matrix, nat.VP_YUV_LIMITED)
            calls.append((lib.vp_op_preprocess_yuv, (ctypes.byref(frames), n, h, w, None, T,
                                                     nat.VP_RESIZE_CENTER_CROP, S, nat._ptr(out), stream), frames))
    state = {"i": 0}

    def run():
        c = calls[state["i"] % len(calls)]
        state["i"] += 1
        nat.check(c[0](*c[1]))
    return run


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def check_bitwise(fmt, clip, h, w):
    """Frame 0 of `clip`: the fused kernel against the RGB kernel on the frame converted on the host."""
    planes = tuple(p[:1] for p in clip)
    host = tuple(p.cpu().numpy() for p in planes)
    matrix = video_utils.yuv_matrix("auto", h, w)
    rgb = torch.from_numpy(yr.yuv_to_rgb(host, fmt, matrix, "limited")).to(planes[0].device)
    got = video_utils.preprocess_yuv_frames(planes, pixel_format=fmt)
    return bool(torch.equal(got, video_utils.preprocess_frames(rgb)))


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", nargs="+", default=["nv12", "i420", "p010"], choices=["nv12", "i420", "p010"])
    ap.add_argument("--rounds", type=int, default=25, help="timed windows per kernel (at least 20)")
    ap.add_argument("--iters", type=int, default=50, help="launches per window")
    ap.add_argument("--pool-mib", type=int, default=768, help="source bytes the launches of a kernel cycle through")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    if args.rounds < 20:
        raise SystemExit("preprocess_yuv_bench: --rounds must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_yuv_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rec = {"tool": "preprocess_yuv_bench", "device": torch.cuda.get_device_name(0), "frames_per_clip": T,
           "target_size": S, "resize_mode": "center_crop", "rounds": args.rounds, "launches_per_window": args.iters,
           "pool_mib": args.pool_mib, "baseline": "preprocess_frames_kernel (packed RGB) on frames of the same size",
           "results": {}}
    ok = True
    for h, w in SIZES:
        res = rec["results"][f"{h}x{w}"] = {}
        for fmt in args.format:
            pools, fns = {}, {}
            out = torch.empty((T, S, S, 3), dtype=torch.uint8, device=dev)
            for k in (fmt, "rgb"):
                clips = max(2, -(-args.pool_mib * (1 << 20) // (T * source_bytes(k, h, w))))
                pools[k] = make_pool(k, h, w, clips, gen, dev)
                fns[k] = launcher(k, pools[k], h, w, out)
            same = check_bitwise(fmt, pools[fmt][0], h, w)
            for k in fns:  # warm-up: every clip of the pool once
                window(fns[k], len(pools[k]))
            ms = {k: [] for k in fns}
            for _ in range(args.rounds):  # alternating, so a drift of the machine falls on both alike
                for k in fns:
                    ms[k].append(window(fns[k], args.iters))
            ratio = statistics.median(ms[fmt]) / statistics.median(ms["rgb"])
            row = dict(summary(ms[fmt]), clips_in_pool=len(pools[fmt]), source_MB_per_clip=round(T * source_bytes(fmt, h, w) / 1e6, 2),
                       rgb=dict(summary(ms["rgb"]), clips_in_pool=len(pools["rgb"]),
                                source_MB_per_clip=round(T * source_bytes("rgb", h, w) / 1e6, 2)),
                       ratio_to_rgb=round(ratio, 4), bitwise_equal_to_rgb_route=same)
            res[fmt] = row
            ok = ok and same and (fmt != "nv12" or ratio <= 1.10)
            print(f"{h}x{w} {fmt}: {row['ms_median']:.4f} ms a clip (min {row['ms_min']:.4f}, max {row['ms_max']:.4f}); "
                  f"rgb {row['rgb']['ms_median']:.4f} ms (min {row['rgb']['ms_min']:.4f}, max {row['rgb']['ms_max']:.4f}); "
                  f"ratio {ratio:.3f}; bitwise {same}", flush=True)
            del pools, fns
            torch.cuda.empty_cache()
    if "nv12" in args.format:
        rec["nv12_within_1.10x_of_rgb"] = all(r["nv12"]["ratio_to_rgb"] <= 1.10 for r in rec["results"].values())
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
