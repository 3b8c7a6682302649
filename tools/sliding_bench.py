"""Sliding windows over one long video: re-encoding every window against per-frame spatial states computed once.

Base bf16, 288 x 288, synthetic weights, one video of 527 frames, windows of T = 16 at stride 1, 4, 8 and 16, in
batches of 32 windows.  Per stride, one batch in the steady state of a stream:

  (a) `apply` on the 32 gathered clips [32, 16, 288, 288, 3]: the only way before `apply_windows`.  The gather of the
      clips is done outside the timed region.
  (b) `encode_frames` on the 32 * stride frames the batch adds, `FrameStates.cat` with the 16 - stride states carried
      over from the batch before, `apply_windows` over the 32 windows.

The window index is a host tensor, as `video_utils.sliding_windows` gives it (range-checked, copied to the device per
call).  Every stride, 16 included, takes the frame gather (`gather_frames_kernel`), the one launch `apply_windows` adds
to `apply`'s; its own time is read from the profiler (class `misc`) and recorded.

One process; (a) and (b) alternate round by round; each round is timed with HIP events over `--iters` calls; the
figures are medians over the rounds, and the spread of a variant is (max - min) / median of its rounds.  The outputs
of (a) and (b) are asserted bitwise equal in the run.  The same run reads the vp_profile_* per-class kernel times of
the spatial half (512 frames, S) and of the temporal half (32 windows: Tm without the gather, G the gather) and prints
the ratio they predict, (S + Tm) / (S * stride / 16 + Tm), beside the ratio measured; and, since 32 * stride frames do not fill the GPU as 512
do, the same ratio with the spatial half's kernel time at the batch's own frame count, (S + Tm) / (S_n + Tm).

Conditions held against (a) in the same run: at stride 16 (the same work) (b) may be slower by no more than the run's
own spread; at stride 1, 4, 8 a measured gain more than 10 % below the predicted one is reported as a finding.

    python tools/sliding_bench.py [--out profiles/sliding_windows/sliding_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import torch  # noqa: E402

from videoprism import encoders, models, params, video_utils  # noqa: E402

T = 16
WINDOWS = 32
STRIDES = (1, 4, 8, 16)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def profiled_ms(eng, fn):
    """Summed kernel milliseconds (HIP events around every launch) of one call of fn, and its per-class split."""
    eng.profile_enable(4096)
    eng.profile_only(None)
    fn()
    torch.cuda.synchronize()
    classes = eng.profile_read()
    eng.profile_enable(0)
    return sum(c["ms"] for c in classes.values()), {k: round(c["ms"], 4) for k, c in classes.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total-frames", type=int, default=527)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spatial-layers", type=int, default=None, help="reduced depth, for a rehearsal")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sliding_bench: no GPU (a measurement needs an MI355X)")
    dev = torch.device("cuda:0")
    cfg = dict(models.CONFIGS["videoprism_v1_base"])
    if args.spatial_layers is not None:
        cfg["num_spatial_layers"] = args.spatial_layers
    model = models.get_model(None, model_fn=lambda: encoders.FactorizedEncoder(**cfg), fprop_dtype=torch.bfloat16)
    var = params.synthetic_params(cfg, seed=0)
    eng = model.engine(var, 0)
    g = torch.Generator(device=dev).manual_seed(0)
    video = torch.rand((args.total_frames, 288, 288, 3), generator=g, device=dev).to(torch.bfloat16)

    # per-class kernel times of the two halves at the bench step (512 frames; 32 windows of them)
    step_frames = video[:WINDOWS * T]
    fs_step = model.encode_frames(var, step_frames)
    idx_step = torch.from_numpy(video_utils.sliding_windows(WINDOWS * T, T, T))
    model.apply_windows(var, fs_step, idx_step)
    spatial_ms, spatial_cls = profiled_ms(eng, lambda: model.encode_frames(var, step_frames))
    windows_ms, temporal_cls = profiled_ms(eng, lambda: model.apply_windows(var, fs_step, idx_step))
    gather_ms = temporal_cls.get("misc", 0.0)  # gather_frames_kernel: the launch apply_windows adds
    assert gather_ms > 0.0, "the frame gather did not run"
    temporal_ms = windows_ms - gather_ms
    del fs_step

    rows = []
    for stride in STRIDES:
        all_windows = video_utils.sliding_windows(args.total_frames, T, stride)
        assert all_windows.shape[0] >= WINDOWS, (stride, all_windows.shape)
        carried_n = T - stride  # states the batch before leaves behind
        span = carried_n + WINDOWS * stride  # frames the 32 windows reach over
        frames = video[:span]
        idx = torch.from_numpy(video_utils.sliding_windows(span, T, stride))  # on the host
        assert idx.shape == (WINDOWS, T)
        clips = frames[idx.long().to(dev)].contiguous()  # (a)'s input, gathered outside the timed region
        carried = model.encode_frames(var, frames[:carried_n])
        new = frames[carried_n:]

        def run_a():
            return model.apply(var, clips)[0]

        def run_b():
            fs = encoders.FrameStates.cat([carried, model.encode_frames(var, new)])
            return model.apply_windows(var, fs, idx)[0]

        out_a, out_b = run_a(), run_b()
        torch.cuda.synchronize()
        assert torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)), f"stride {stride}: outputs differ"
        del out_a, out_b
        for _ in range(args.warmup):
            run_a()
            run_b()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):  # alternating rounds
            ta.append(timed(run_a, args.iters))
            tb.append(timed(run_b, args.iters))
        ma, mb = statistics.median(ta), statistics.median(tb)
        spread_a, spread_b = (max(ta) - min(ta)) / ma, (max(tb) - min(tb)) / mb
        predicted = (spatial_ms + temporal_ms) / (spatial_ms * stride / T + temporal_ms)
        spatial_n_ms, _ = profiled_ms(eng, lambda: model.encode_frames(var, new))
        predicted_n = (spatial_ms + temporal_ms) / (spatial_n_ms + temporal_ms)
        measured = ma / mb
        row = dict(stride=stride, new_frames_per_batch=WINDOWS * stride, reencode_ms=round(ma, 3),
                   windows_ms=round(mb, 3), reencode_rounds_ms=[round(t, 3) for t in ta],
                   windows_rounds_ms=[round(t, 3) for t in tb], spread_reencode=round(spread_a, 4),
                   spread_windows=round(spread_b, 4), ratio_measured=round(measured, 3),
                   ratio_predicted=round(predicted, 3), profile_spatial_half_at_size_ms=round(spatial_n_ms, 3),
                   ratio_predicted_at_size=round(predicted_n, 3), outputs_bitwise_equal=True)
        if stride == T:
            row["slower_by"] = round(mb / ma - 1.0, 4)
            row["within_spread"] = bool(mb / ma - 1.0 <= max(spread_a, spread_b))
        else:
            row["gain_short_of_predicted"] = round(1.0 - measured / predicted, 4)
            row["finding"] = bool(measured < 0.9 * predicted)
        rows.append(row)
        print(f"stride {stride:2d}: re-encode {ma:7.3f} ms (spread {spread_a:.2%})  states+windows {mb:7.3f} ms "
              f"(spread {spread_b:.2%})  ratio measured {measured:.2f}x  predicted {predicted:.2f}x  "
              f"(at {WINDOWS * stride} frames' own kernel times {predicted_n:.2f}x)", flush=True)
        del clips, carried

    rec = dict(tool="sliding_bench", model="videoprism_v1_base", fprop_dtype="bfloat16", frame_size=288,
               total_frames=args.total_frames, num_frames=T, windows_per_batch=WINDOWS, rounds=args.rounds,
               iters=args.iters, num_spatial_layers=cfg["num_spatial_layers"], device=torch.cuda.get_device_name(0),
               profile_spatial_half_ms=round(spatial_ms, 3), profile_temporal_half_ms=round(temporal_ms, 3),
               profile_gather_ms=round(gather_ms, 4),
               profile_spatial_classes_ms=spatial_cls, profile_temporal_classes_ms=temporal_cls, strides=rows)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
