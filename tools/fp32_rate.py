"""Throughput of the fp32 forward (fprop_dtype=None: the reference's default precision, models.py:268-303):
Base (or Large, or `giant`: videoprism_v1_giant, which has no checkpoint name) at B clips x 16 x 288 x 288 on one
GPU, with the per-class kernel breakdown from the library's HIP-event profiler.  Measurement only (the bench's
headline is bf16).

  python tools/fp32_rate.py [videoprism_public_v1_base | videoprism_public_v1_large | giant] [B] [steps]

The video-text and classifier models, with synthetic weights at full depth: `lvt_large`, `giant_lvt` (video + text,
Q = 32 texts of L = 64 tokens) and `giant_vc` (400 classes).  For these the result also holds the pooler's passes
(pool_logits, pool_softmax_wsum, ln_l2_rows) timed one at a time on tokens of the forward's shape, as GB/s of the
token bytes each one streams, and -- for a 'primer_hybrid' text tower -- the LayerNorm and LayerNorm-residual
launches of one text layer beside the tower's time per layer."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import torch  # noqa: E402

from videoprism import _native as nat  # noqa: E402
from videoprism import models, params  # noqa: E402

HEADS = {"lvt_large": lambda: models.videoprism_lvt_v1_large(), "giant_lvt": lambda: models.videoprism_lvt_v1_giant(),
         "giant_vc": lambda: models.videoprism_vc_v1_giant(400)}
Q, L = 32, 64


def _kernels(br):
    return {k: {"ms": round(v["ms"], 3), "launches": v["launches"],
                "tflops": round(v["flops"] / v["ms"] / 1e9, 1) if v["flops"] else None}
            for k, v in sorted(br.items(), key=lambda kv: -kv[1]["ms"])}


def _timed(fn, reps=20):
    """Mean milliseconds of fn() over reps launches between two events, after two warm-up calls."""
    fn()
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def pooler_passes(D, H, G, S):
    """The pooler's streaming passes over fp32 tokens [G * S, D], one kernel sequence at a time."""
    x = torch.randn(G * S, D, device="cuda:0")
    U = torch.randn(H, D, device="cuda:0") / D ** 0.5
    C = nat.dev_pool_chunks(S)
    logits, stats = torch.empty(G, H, S, device="cuda:0"), torch.empty(G * H, 2, device="cuda:0")
    zpart, z = torch.empty(G, C, H, D, device="cuda:0"), torch.empty(G, H, D, device="cuda:0")
    pooled, out = torch.randn(G, D, device="cuda:0"), torch.empty(G, D, device="cuda:0")
    g1p, beta = torch.ones(D, device="cuda:0"), torch.zeros(D, device="cuda:0")
    gb = G * S * D * 4 / 1e9
    ms = {"pool_logits": _timed(lambda: nat.dev_pool_logits(x, S, U, None, logits, wide=True)),
          "pool_softmax_wsum": _timed(lambda: nat.dev_pool_softmax_wsum(x, G, S, H, logits, stats, zpart, z, wide=True)),
          "ln_l2_rows": _timed(lambda: nat.dev_ln_l2_rows(pooled, D, G, D, g1p, beta, True, out, wide=True))}
    return {"D": D, "heads": H, "groups": G, "rows_per_group": S,
            "pool_logits": {"ms": round(ms["pool_logits"], 4), "GBps": round(gb / ms["pool_logits"] * 1e3, 1)},
            "pool_softmax_wsum": {"ms": round(ms["pool_softmax_wsum"], 4),
                                  "GBps": round(gb / ms["pool_softmax_wsum"] * 1e3, 1)},
            "ln_l2_rows": {"ms": round(ms["ln_l2_rows"], 4)}}


def text_layer_norms(D, rows):
    """One primer text layer's LayerNorm launches on the fp32 stream [rows, D]: 2 x layernorm, 2 x layernorm_residual."""
    xs, y = torch.randn(rows, D, device="cuda:0"), torch.randn(rows, D, device="cuda:0")
    g1p, beta, pad = torch.ones(D, device="cuda:0"), torch.zeros(D, device="cuda:0"), torch.zeros(rows, device="cuda:0")
    ln = _timed(lambda: nat.op_layernorm(xs, g1p, beta))
    lnr = _timed(lambda: nat.dev_layernorm_residual(y, g1p, beta, xs, pad))
    return {"rows": rows, "layernorm_ms": round(ln, 4), "layernorm_residual_ms": round(lnr, 4),
            "four_launches_ms": round(2 * ln + 2 * lnr, 4)}


def heads_main(name, B, steps):
    model = HEADS[name]()
    var = params.synthetic_params(model.config(), seed=0, specs=model.param_specs())
    eng = model.engine(var, 0)
    del var
    cfg = model.config()
    D, H = cfg["model_dim"], cfg["num_heads"]
    video = torch.rand((B, 16, 288, 288, 3), device="cuda:0")
    clip = name != "giant_vc"
    if clip:
        ids = torch.randint(0, cfg["vocabulary_size"], (Q, L), device="cuda:0", dtype=torch.int32)
        pads = torch.zeros((Q, L), device="cuda:0")
        pads[::2, L // 2:] = 1.0

    def step():
        if clip:
            eng.encode_video(video, want_frames=True)
            eng.encode_text(ids, pads)
        else:
            eng.forward(video)

    step()
    torch.cuda.synchronize()
    eng.profile_enable(4096)
    step()
    torch.cuda.synchronize()
    br = eng.profile_read()
    eng.profile_enable(0)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    res = {"model": name, "dtype": "f32", "B": B, "texts": [Q, L] if clip else None, "ms_per_step": round(dt * 1e3, 2),
           "clips_per_s": round(B / dt, 2), "kernels": _kernels(br),
           "pooler_passes_clip": pooler_passes(D, H, B, 16 * 256)}
    if clip:
        res["pooler_passes_frames"] = pooler_passes(D, H, B * 16, 256)
        layers = cfg["num_unimodal_layers"]
        res["text_tower_ms_per_layer"] = round(br["text_tower"]["ms"] / layers, 4)
        if cfg.get("norm_policy") == "primer_hybrid":
            res["text_layer_norms"] = text_layer_norms(D, (Q * (L + 1) + 255) // 256 * 256)
    print(json.dumps(res, indent=1))


def main(name="videoprism_public_v1_base", B=4, steps=3):
    if name in HEADS:
        return heads_main(name, B, steps)
    cfg_key = {"videoprism_public_v1_base": "videoprism_v1_base",
               "videoprism_public_v1_large": "videoprism_v1_large", "giant": "videoprism_v1_giant"}[name]
    cfg = dict(models.CONFIGS[cfg_key])
    # fp32; Giant is in no checkpoint table (as in the reference), so it comes from its builder
    model = models.get_model(None, model_fn=models.videoprism_v1_giant) if name == "giant" else models.get_model(name)
    var = params.synthetic_params(cfg, seed=0)
    eng = model.engine(var, 0)
    video = torch.rand((B, 16, 288, 288, 3), device="cuda:0")
    out = torch.empty((B, 16 * 256, cfg["model_dim"]), device="cuda:0")
    eng.forward(video, out=out)
    torch.cuda.synchronize()
    eng.profile_enable(512)
    eng.forward(video, out=out)
    torch.cuda.synchronize()
    br = eng.profile_read()
    eng.profile_enable(0)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.forward(video, out=out)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    gpc = 973.29 if "base" in name else None
    res = {"model": name, "dtype": "f32", "B": B, "ms_per_step": round(dt * 1e3, 2), "clips_per_s": round(B / dt, 2),
           "tflops_whole_forward": round(B * gpc / dt / 1e3, 1) if gpc else None, "kernels": _kernels(br)}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(*(sys.argv[1:2] or []), *([int(a) for a in sys.argv[2:4]]))
