"""Views in the frame ingest (csrc/preprocess.hip, the VIEWS instantiations) beside the plain kernels and the parent
revision's library: 32 videos x 16 frames of 720 x 1280 already on the device, S = 288, packed RGB and NV12.

  (a) preprocess    vp_op_preprocess_frames / vp_op_preprocess_yuv (centre crop) of this build against the parent
                    library's, loaded side by side (tools/ab_build.sh builds it): the existing kernels did not move
  (b) centre view   the same pixels in and out through one centre view per video (vp_op_preprocess_views /
                    vp_op_preprocess_yuv_views), compared bitwise with (a) and timed against (a) on the parent
  (c) multi_view    4 temporal x 3 spatial views of 8 frames per video in one launch (96 output frames a video),
                    as time per output frame beside (b)'s
  (d) random crop   one random-resized-crop view (and a coin-flip mirror) per video, fixed seed, beside the Base bf16
                    vp_forward step it feeds, as tools/preprocess_bench.py does

HIP events around windows of `--iters` launches; the arms alternate for `--rounds` rounds, so a drift of the machine
falls on all alike.  The launches call the C entry points with arguments built once, so a window measures the kernel
and not Python.  Conditions: the medians of (a) and (b) on this build must not exceed the parent's slowest round of
(a) in the same session (the parent's own min-max spread is the only noise figure that belongs to the session), and
(d) must add no more than 10 % to the forward step.  (c) is recorded.

    bash tools/ab_build.sh HEAD~1 parent
    python tools/preprocess_views_bench.py --parent .ab/parent/videoprism-mlx_amd/videoprism/libvideoprism_hip.so \\
        [--out profiles/ingest_views/bench.json] [--txt profiles/ingest_views/bench.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from videoprism import _native as nat  # noqa: E402
from videoprism import models, params, video_utils  # noqa: E402

B, T, H, W, S = 32, 16, 720, 1280, 288
ENTRIES = ("vp_op_preprocess_frames", "vp_op_preprocess_yuv")


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5)}


def table(views, idx, dev):
    """(table [B*V, 9], frame indices [B*V*T'] into the B*T flattened frames) on the device, the [V, 9] views and
    [V, T'] indices shared by all videos or given per video."""
    views, idx = np.asarray(views), np.asarray(idx)
    if views.ndim == 2:
        views, idx = np.broadcast_to(views, (B,) + views.shape), np.broadcast_to(idx, (B,) + idx.shape)
    flat = idx + np.arange(B)[:, None, None] * T
    return (torch.from_numpy(np.ascontiguousarray(views, dtype=np.int32).reshape(-1, 9)).to(dev),
            torch.from_numpy(np.ascontiguousarray(flat, dtype=np.int32).reshape(-1)).to(dev), views.shape[1], idx.shape[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent revision's libvideoprism_hip.so (tools/ab_build.sh)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20, help="launches per window")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--txt", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_views_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    this, parent = nat.load(), ctypes.CDLL(args.parent)
    for name in ENTRIES:
        f = getattr(parent, name)
        f.restype, f.argtypes = nat._SIGNATURES[name]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    stream = nat._stream()
    p = nat._ptr
    F = B * T
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    centre = table(video_utils.view_table(H, W, target_size=S), np.arange(T)[None], dev)
    mv_idx, mv_views = video_utils.multi_view(T, H, W, num_frames=8, temporal_views=4, spatial_views=3, target_size=S)
    multi = table(mv_views, mv_idx, dev)
    boxes = video_utils.random_resized_crop(H, W, B, rng=rng)
    crops = video_utils.view_table(H, W, boxes=boxes, target_size=S, resize_mode="resize", flip=rng.random(B) < 0.5)
    crop = table(crops[:, None], np.broadcast_to(np.arange(T), (B, 1, T)), dev)

    name = "videoprism_public_v1_base"
    cfg = dict(models.CONFIGS["videoprism_v1_base"])
    eng = models.get_model(name, fprop_dtype=torch.bfloat16).engine(params.synthetic_params(cfg, seed=0), 0)
    emb = torch.empty((B, T * 256, cfg["model_dim"]), dtype=torch.bfloat16, device=dev)

    rec = {"tool": "preprocess_views_bench", "device": torch.cuda.get_device_name(0), "videos": B, "frames_per_video": T,
           "source": f"{H}x{W}", "target_size": S, "rounds": args.rounds, "launches_per_window": args.iters,
           "parent": args.parent, "results": {}}
    ok = True
    for fmt in ("rgb", "nv12"):
        if fmt == "rgb":
            src = torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
            plain = lambda lib, out: (lib.vp_op_preprocess_frames, (p(src), F, H, W, 3 * W, 3 * W * H, None, F,  # noqa: E731
                                                                   nat.VP_RESIZE_CENTER_CROP, 0, S, p(out), stream))
            viewed = lambda tab, out: (this.vp_op_preprocess_views, (p(src), F, H, W, 3 * W, 3 * W * H, p(tab[1]),  # noqa: E731
                                                                     p(tab[0]), B * tab[2], tab[3], 0, S, p(out), stream))
        else:
            planes = (torch.randint(0, 256, (F, H, W), generator=g, device=dev, dtype=torch.uint8),
                      torch.randint(0, 256, (F, H // 2, W // 2, 2), generator=g, device=dev, dtype=torch.uint8))
            frames, *_ = nat.yuv_frames(planes, nat.VP_YUV_NV12, nat.VP_YUV_BT709, nat.VP_YUV_LIMITED)
            plain = lambda lib, out: (lib.vp_op_preprocess_yuv, (ctypes.byref(frames), F, H, W, None, F,  # noqa: E731
                                                                nat.VP_RESIZE_CENTER_CROP, S, p(out), stream))
            viewed = lambda tab, out: (this.vp_op_preprocess_yuv_views, (ctypes.byref(frames), F, H, W, p(tab[1]),  # noqa: E731
                                                                         p(tab[0]), B * tab[2], tab[3], S, p(out), stream))
        outs = {k: torch.empty((F, S, S, 3), dtype=torch.uint8, device=dev) for k in ("a_parent", "a_this", "b_centre", "d_crop")}
        outs["c_multi"] = torch.empty((multi[0].shape[0] * multi[3], S, S, 3), dtype=torch.uint8, device=dev)
        calls = {"a_parent": plain(parent, outs["a_parent"]), "a_this": plain(this, outs["a_this"]),
                 "b_centre": viewed(centre, outs["b_centre"]), "c_multi": viewed(multi, outs["c_multi"]),
                 "d_crop": viewed(crop, outs["d_crop"])}
        fns = {k: (lambda c=c: nat.check(c[0](*c[1]))) for k, c in calls.items()}
        for f in fns.values():  # warm-up, and the outputs the comparisons read
            f()
            f()
        torch.cuda.synchronize()
        same = {k: bool(torch.equal(outs[k], outs["a_parent"])) for k in ("a_this", "b_centre")}
        fns["vp_forward"] = lambda: eng.forward(outs["d_crop"].view(B, T, S, S, 3), out=emb)
        fns["vp_forward"]()
        ms = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, f in fns.items():
                ms[k].append(window(f, 2 if k == "vp_forward" else args.iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        lo, hi = min(ms["a_parent"]), max(ms["a_parent"])
        frames_out = {k: outs[k].shape[0] for k in outs}
        res = rec["results"][fmt] = {k: dict(summary(v), output_frames=frames_out.get(k)) for k, v in ms.items()}
        res["bitwise_equal_to_parent"] = same
        res["a_this_over_parent_median"] = round(med["a_this"] / med["a_parent"], 4)
        res["b_centre_over_parent_median"] = round(med["b_centre"] / med["a_parent"], 4)
        res["a_within_parent_spread"] = med["a_this"] <= hi
        res["b_within_parent_spread"] = med["b_centre"] <= hi
        res["c_us_per_output_frame"] = round(med["c_multi"] / frames_out["c_multi"] * 1e3, 4)
        res["b_us_per_output_frame"] = round(med["b_centre"] / F * 1e3, 4)
        res["d_share_of_forward"] = round(med["d_crop"] / med["vp_forward"], 4)
        res["d_within_10_percent_of_forward"] = med["d_crop"] <= 0.10 * med["vp_forward"]
        ok = ok and all(same.values()) and res["a_within_parent_spread"] and res["b_within_parent_spread"] and \
            res["d_within_10_percent_of_forward"]
        say(f"{fmt} (a) preprocess, parent: {med['a_parent']:.4f} ms (rounds {lo:.4f} .. {hi:.4f}); this build: "
            f"{med['a_this']:.4f} ms (rounds {min(ms['a_this']):.4f} .. {max(ms['a_this']):.4f}), ratio "
            f"{res['a_this_over_parent_median']:.4f}, bitwise {same['a_this']}: "
            f"{'within' if res['a_within_parent_spread'] else 'OUTSIDE'} the parent's spread")
        say(f"{fmt} (b) one centre view per video: {med['b_centre']:.4f} ms (rounds {min(ms['b_centre']):.4f} .. "
            f"{max(ms['b_centre']):.4f}), ratio to the parent's (a) {res['b_centre_over_parent_median']:.4f}, bitwise "
            f"{same['b_centre']}: {'within' if res['b_within_parent_spread'] else 'OUTSIDE'} the parent's spread")
        say(f"{fmt} (c) multi_view 4 x 3 x 8 frames: {med['c_multi']:.4f} ms for {frames_out['c_multi']} frames = "
            f"{res['c_us_per_output_frame']:.3f} us a frame; (b) is {res['b_us_per_output_frame']:.3f} us a frame")
        say(f"{fmt} (d) one random resized crop per video: {med['d_crop']:.4f} ms (rounds {min(ms['d_crop']):.4f} .. "
            f"{max(ms['d_crop']):.4f}) = {100 * res['d_share_of_forward']:.2f} % of the forward step "
            f"({med['vp_forward']:.2f} ms, {name} bf16): "
            f"{'within' if res['d_within_10_percent_of_forward'] else 'OUTSIDE'} 10 %")
        del outs, calls, fns
        torch.cuda.empty_cache()
    rec["ok"] = ok
    print(json.dumps(rec), flush=True)
    for path, text in ((args.out, json.dumps(rec, indent=1) + "\n"), (args.txt, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
