"""Same-process A/B of one kernel entry between this tree's product library and another revision's
(built by tools/ab_build.sh): both libraries are loaded side by side (ctypes, RTLD_LOCAL), fed the same
device buffers, timed in interleaved rounds, and their outputs compared bitwise.

  python tools/ab_lib.py tattn .ab/old/videoprism-mlx_amd/videoprism/libvideoprism_hip.so
  python tools/ab_lib.py gemm old=.ab/old/videoprism-mlx_amd/videoprism/libvideoprism_hip.so [NAME=LIB.so ...]
"""
import ctypes
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]
import torch  # noqa: E402

from videoprism import _native as nat  # noqa: E402


def timeit(fn, iters=20, warm=3):
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


def bind(lib):
    f = lib.vp_dev_gemm_tattn
    f.restype, f.argtypes = nat._SIGNATURES["vp_dev_gemm_tattn"]
    return f


def tattn(other):
    """The fused temporal attention launches (vp_dev_gemm_tattn) at the bench shape."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    M, D, H = 131072, 768, 12
    x = (torch.rand((M, D), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand((3 * D, D), generator=g, device=dev) * 2 - 1) / D ** 0.5).to(torch.bfloat16)
    wqk, wv = w[:2 * D].contiguous(), w[2 * D:].contiguous()
    b = torch.randn(3 * D, generator=g, device=dev) * 0.1
    c = torch.randn(3 * D, generator=g, device=dev) * 0.1
    rs = torch.stack([torch.rand(M, generator=g, device=dev) + 0.5, torch.randn(M, generator=g, device=dev) * 0.1],
                     1).contiguous()
    libs = {"this": bind(nat.load()), "other": bind(ctypes.CDLL(other))}
    p = {k: torch.empty(M // 16 * H * 256, device=dev, dtype=torch.bfloat16) for k in libs}
    o = {k: torch.empty(M, D, device=dev, dtype=torch.bfloat16) for k in libs}
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def qk(k):
        assert libs[k](0, ptr(x), ptr(wqk), M, D, ptr(p[k]), ptr(b), ptr(rs), ptr(c), None, H, 50.0, st()) == 0

    def vv(k):
        assert libs[k](1, ptr(x), ptr(wv), M, D, ptr(o[k]), ptr(b[2 * D:]), ptr(rs), ptr(c[2 * D:]), ptr(p[k]), H,
                       50.0, st()) == 0
    for k in libs:
        qk(k)
        vv(k)
    torch.cuda.synchronize()
    print("bitwise this == other: P", bool(torch.equal(p["this"], p["other"])), "O",
          bool(torch.equal(o["this"], o["other"])), flush=True)
    fns = {f"qk-{k}": (lambda k=k: qk(k)) for k in libs}
    fns.update({f"v-{k}": (lambda k=k: vv(k)) for k in libs})
    res = {k: [] for k in fns}
    for _ in range(4):
        for k, f in fns.items():
            res[k].append(timeit(f))
    print("tattn:", " | ".join(f"{k} {min(v)*1e3:7.1f} us" for k, v in res.items()), flush=True)


def spatial(other):
    """The spatial attention (S = 256, 12 heads, 512 frames: the bench shape) over the row-major
    q|k|v (vp_op_attention) and the row-blocked one (vp_dev_attention_spatial_blk), plus a padded
    batch (the masked kernel) and an item count that is not a multiple of the grid: bitwise this vs
    other, interleaved timing."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    H, D = 12, 768
    libs = {"this": nat.load(), "other": ctypes.CDLL(other)}
    for lib in libs.values():
        for name in ("vp_op_attention", "vp_dev_attention_spatial_blk"):
            f = getattr(lib, name)
            f.restype, f.argtypes = nat._SIGNATURES[name]
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for nseq, blk, padded in ((512, True, False), (512, False, False), (37, True, False), (100, True, False), (16, False, True),
                              (16, True, True)):
        qkv = torch.randn((nseq * 256, 3 * D), generator=g, device=dev)
        qkv[:, :D] *= 0.125
        qkv = qkv.to(torch.bfloat16)
        pad = None
        if padded:
            pad = torch.zeros(nseq * 256, device=dev)
            pad[5 * 256 + 200: 6 * 256] = 1.0
        outs = {k: torch.empty((nseq * 256, D), device=dev, dtype=torch.bfloat16) for k in libs}

        def run(k):
            if blk:
                assert libs[k].vp_dev_attention_spatial_blk(ptr(qkv), ptr(outs[k]), nseq, H, 50.0, ptr(pad), st()) == 0
            else:
                assert libs[k].vp_op_attention(1, ptr(qkv), ptr(outs[k]), nseq, 256, H, 50.0, ptr(pad), st()) == 0
        for k in libs:
            run(k)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["this"], outs["other"]))
        res = {k: [] for k in libs}
        for _ in range(5):
            for k in libs:
                res[k].append(timeit(lambda k=k: run(k)))
        print(f"spatial nseq={nseq} blk={blk} padded={padded}: bitwise this == other {same}; " + " | ".join(
            f"{k} {min(v)*1e3:7.1f} us" for k, v in res.items()), flush=True)


def attention(other):
    """vp_op_attention (bf16, 12 heads unless stated) at the small shapes the whole forwards do not reach: key
    paddings on the spatial, sequence-packed and temporal kernels (a partly and a fully padded sequence), partial
    blocks, and the long kernel with and without a tail.  Bitwise this vs other; interleaved timing with the other
    library loaded a second time (from a copy of the file) beside it, so other vs other2 is the run's own spread."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    tmp = tempfile.NamedTemporaryFile(suffix=".so", delete=False).name
    shutil.copy(other, tmp)
    libs = {"this": nat.load(), "other": ctypes.CDLL(other), "other2": ctypes.CDLL(tmp)}
    os.unlink(tmp)
    for lib in libs.values():
        lib.vp_op_attention.restype, lib.vp_op_attention.argtypes = nat._SIGNATURES["vp_op_attention"]
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    cases = [(256, 3, 12, True)] + [(S, 11, 12, p) for S in (40, 64, 130) for p in (True, False)]
    cases += [(8, 11, 12, True), (16, 11, 12, True), (300, 1, 2, False), (512, 1, 2, False)]
    for S, nseq, H, padded in cases:
        D = 64 * H
        qkv = torch.randn((nseq * S, 3 * D), generator=g, device=dev)
        qkv[:, :D] *= 0.125
        qkv = qkv.to(torch.bfloat16)
        pad = None
        if padded:  # sequence 1 partly padded, the last one fully
            pad = torch.zeros(nseq * S, device=dev)
            pad[S + S // 2 + 1: 2 * S] = 1.0
            pad[(nseq - 1) * S:] = 1.0
        outs = {k: torch.full((nseq * S, D), -1.0, device=dev, dtype=torch.bfloat16) for k in libs}

        def run(k):
            assert libs[k].vp_op_attention(1, ptr(qkv), ptr(outs[k]), nseq, S, H, 50.0, ptr(pad), st()) == 0
        for k in libs:
            run(k)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["this"].view(torch.int16), outs["other"].view(torch.int16)))
        res = {k: [] for k in libs}
        for _ in range(5):
            for k in libs:
                res[k].append(timeit(lambda k=k: run(k)))
        print(f"attention S={S} nseq={nseq} heads={H} padded={padded}: bitwise this == other {same}; " + " | ".join(
            f"{k} {min(v)*1e3:7.1f} us" for k, v in res.items()), flush=True)


def pooler(other, control=False):
    """The pooler's streaming passes one at a time (vp_dev_pool_logits, vp_dev_pool_softmax_wsum; the *_wide entry
    where the plain one refuses the width) and the head's training ops (vp_op_probe_forward, then
    vp_op_probe_backward: the logits and all 14 gradients) at the first five shapes of tests/test_gpu_probe.py and at
    Base's head shape.  Bitwise this vs other; interleaved timing with the other library loaded a second time, so
    other vs other2 is the run's own spread, and `over` is min(this) - min(other) set against it.  A third argument
    `control` runs the same with a copy of the other library in this tree's place."""
    from videoprism.probe import AttentiveProbe
    dev = torch.device("cuda:0")
    if control:  # a copy of the other library stands in for this tree's: what the harness itself adds to "this"
        nat._LIB_PATH = tempfile.NamedTemporaryFile(suffix=".so", delete=False).name
        shutil.copy(other, nat._LIB_PATH)
    tmp = tempfile.NamedTemporaryFile(suffix=".so", delete=False).name
    shutil.copy(other, tmp)
    libs = {"this": nat.load(), "other": ctypes.CDLL(other), "other2": ctypes.CDLL(tmp)}
    os.unlink(tmp)
    if control:
        os.unlink(nat._LIB_PATH)
    names = ("vp_dev_pool_logits", "vp_dev_pool_logits_wide", "vp_dev_pool_softmax_wsum",
             "vp_dev_pool_softmax_wsum_wide", "vp_op_probe_forward", "vp_op_probe_backward")
    for lib in libs.values():
        for name in names:
            f = getattr(lib, name)
            f.restype, f.argtypes = nat._SIGNATURES[name]
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def ab(label, run, outs):
        """run(k) fills outs[k] (a list of tensors) through library k."""
        for k in libs:
            run(k)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(outs["this"], outs["other"]))
        res = {k: [] for k in libs}
        for _ in range(5):
            for k in libs:
                res[k].append(timeit(lambda k=k: run(k)))
        t = {k: min(v) * 1e3 for k, v in res.items()}
        over, spread = t["this"] - t["other"], abs(t["other"] - t["other2"])
        print(f"{label}: bitwise this == other {same}; " + " | ".join(f"{k} {v:8.1f} us" for k, v in t.items()) +
              f" | over {over:+7.1f} us, spread {spread:6.1f} us: {'within' if over <= spread else 'OUTSIDE'}",
              flush=True)

    cases = [(False, 1, 40, 128, 2, 1), (False, 3, 300, 384, 6, 5), (False, 2, 257, 1408, 16, 70),
             (True, 2, 512, 256, 4, 3), (True, 3, 300, 384, 6, 5), (True, 32, 4096, 768, 12, 400)]
    for bf16, B, S, D, H, C in cases:
        shape = f"{'bf16' if bf16 else 'fp32'} B={B} S={S} D={D} H={H}"
        g = torch.Generator(device=dev).manual_seed(1000 * D + 10 * S + B)
        x = torch.randn((B * S, D), generator=g, device=dev).to(torch.bfloat16 if bf16 else torch.float32)
        U = torch.randn((H, D), generator=g, device=dev) / D ** 0.5
        Ut = torch.from_numpy(nat.dev_pool_split_u(U.cpu().numpy()).view("int16")).to(dev) if bf16 else None
        dt = nat._prec(x)
        lg = {k: [torch.full((B, H, S), -1.0, device=dev)] for k in libs}
        fn = "vp_dev_pool_logits" + ("_wide" if D > 1024 else "")
        ab(f"pool_logits {shape}", lambda k: _ok(getattr(libs[k], fn)(ptr(x), dt, B * S, S, D, ptr(U), ptr(Ut), H,
                                                                       ptr(lg[k][0]), st())), lg)
        Cn = nat.dev_pool_chunks(S)
        zs = {k: [torch.full((B * H, 2), -1.0, device=dev), torch.full((B, Cn, H, D), -1.0, device=dev),
                  torch.full((B, H, D), -1.0, device=dev)] for k in libs}
        fn2 = "vp_dev_pool_softmax_wsum" + ("_wide" if D > 1024 or D % 256 else "")
        ab(f"pool_softmax_wsum {shape}",
           lambda k: _ok(getattr(libs[k], fn2)(ptr(x), dt, B, S, D, H, ptr(lg["this"][0]), ptr(zs[k][0]), ptr(zs[k][1]),
                                               ptr(zs[k][2]), st())), zs)

        probe = AttentiveProbe(D, H, C, device=dev, seed=0)
        tensors = {m: probe.get_parameter(path).detach() for m, path in nat.PROBE_LEAVES}
        dims, params = nat.vp_probe_dims(D, H, C), nat._probe_struct(tensors)
        dlogits = torch.randn((B, C), generator=g, device=dev)
        need = nat.op_probe_workspace_bytes(D, H, C, B, S)
        ws = {k: torch.empty(need, dtype=torch.uint8, device=dev) for k in libs}
        out = {k: [torch.full((B, C), -1.0, device=dev)] + [torch.full_like(tensors[m], -1.0) for m, _ in nat.PROBE_LEAVES]
               for k in libs}
        gr = {k: nat._probe_struct(dict(zip((m for m, _ in nat.PROBE_LEAVES), out[k][1:]))) for k in libs}

        def fwd(k):
            _ok(libs[k].vp_op_probe_forward(ctypes.byref(dims), ctypes.byref(params), ptr(x), dt, B, S, ptr(out[k][0]),
                                            None, ptr(ws[k]), need, st()))

        def both(k):
            fwd(k)
            _ok(libs[k].vp_op_probe_backward(ctypes.byref(dims), ctypes.byref(params), ptr(x), dt, B, S, ptr(dlogits),
                                             ctypes.byref(gr[k]), ptr(ws[k]), need, st()))
        both("this")  # every gradient written before the forward-only comparison reads the lists
        ab(f"probe forward+backward {shape}", both, out)
        ab(f"probe forward {shape}", fwd, out)


def gemm(others, rounds=7):
    """The forward's 4-wave GEMM launches at the bench shapes (Base, B = 32: M = 131072) on random operands:
    ffn_layer1 (EPI 16, no padded rows), ffn_layer2 (17), the spatial q|k|v (19), post (10), the two fused
    temporal launches (14, 15) and the patch embedding from 512 frames.  `others`: NAME=LIB.so ...; every
    library is loaded beside this tree's, fed the same buffers, compared bitwise with this tree's output and
    timed in interleaved rounds (median and min per arm)."""
    import statistics
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    libs = {"this": nat.load()}
    for spec in others:
        name, path = spec.split("=", 1)
        libs[name] = ctypes.CDLL(path)
    names = ("vp_dev_gemm_ln", "vp_dev_gemm_tattn", "vp_dev_patch_embed")
    for lib in libs.values():
        for n in names:
            f = getattr(lib, n)
            f.restype, f.argtypes = nat._SIGNATURES[n]
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    M, D, F, H = 131072, 768, 3072, 12

    def ab(label, run, outs, flop):
        for k in libs:
            run(k)
        torch.cuda.synchronize()
        same = {k: all(torch.equal(a, b) for a, b in zip(outs["this"], outs[k])) for k in libs if k != "this"}
        res = {k: [] for k in libs}
        for _ in range(rounds):
            for k in libs:
                res[k].append(timeit(lambda k=k: run(k)))
        wins = {k: sum(a < b for a, b in zip(res["this"], res[k])) for k in libs if k != "this"}
        print(f"{label}: bitwise this == " + " ".join(f"{k}:{v}" for k, v in same.items()) + " | " + " | ".join(
            f"{k} median {statistics.median(v)*1e3:7.1f} min {min(v)*1e3:7.1f} us ({flop/min(v)/1e9:6.1f} TF)"
            for k, v in res.items()) + " | rounds this faster: " + " ".join(f"{k} {v}/{rounds}" for k, v in wins.items()),
              flush=True)

    rs = torch.stack([torch.rand(M, generator=g, device=dev) + 0.5, torch.randn(M, generator=g, device=dev) * 0.1],
                     1).contiguous()
    x = (torch.rand((M, D), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    for label, N, K, epi in (("ffn1 <16,nopad,S2>", F, D, 16), ("ffn2 <17,S3>", D, F, 17), ("qkv <19,S3>", 3 * D, D, 19),
                             ("post <10,S3>", D, D, 10)):
        a = x if K == D else (torch.rand((M, K), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
        w = ((torch.rand((N, K), generator=g, device=dev) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
        b = torch.randn(N, generator=g, device=dev) * 0.1
        c = torch.randn(N, generator=g, device=dev) * 0.1
        resid = epi in (17, 10)
        r0 = torch.randn((M, N), generator=g, device=dev).to(torch.bfloat16) if resid else None
        outs = {k: [torch.empty((M, N), device=dev, dtype=torch.bfloat16)] +
                ([torch.empty((N // 128, M, 2), device=dev)] if resid else []) for k in libs}

        def run(k, a=a, w=w, b=b, c=c, r0=r0, N=N, K=K, epi=epi, outs=outs, resid=resid):
            _ok(libs[k].vp_dev_gemm_ln(epi, ptr(a), ptr(w), M, N, K, ptr(outs[k][0]), ptr(b), ptr(r0), None, 0, None,
                                       ptr(rs), ptr(c), ptr(outs[k][1]) if resid else None, st()))
        ab(label, run, outs, 2.0 * M * N * K)
        del a, w, outs, r0

    w = ((torch.rand((3 * D, D), generator=g, device=dev) * 2 - 1) / D ** 0.5).to(torch.bfloat16)
    wqk, wv = w[:2 * D].contiguous(), w[2 * D:].contiguous()
    b = torch.randn(3 * D, generator=g, device=dev) * 0.1
    c = torch.randn(3 * D, generator=g, device=dev) * 0.1
    p = {k: [torch.empty(M // 16 * H * 256, device=dev, dtype=torch.bfloat16)] for k in libs}
    o = {k: [torch.empty(M, D, device=dev, dtype=torch.bfloat16)] for k in libs}
    ab("tattn qk <14,S3>", lambda k: _ok(libs[k].vp_dev_gemm_tattn(0, ptr(x), ptr(wqk), M, D, ptr(p[k][0]), ptr(b), ptr(rs),
                                                                   ptr(c), None, H, 50.0, st())), p, 2.0 * M * 2 * D * D)
    ab("tattn v <15,S3>", lambda k: _ok(libs[k].vp_dev_gemm_tattn(1, ptr(x), ptr(wv), M, D, ptr(o[k][0]), ptr(b[2 * D:]),
                                                                  ptr(rs), ptr(c[2 * D:]), ptr(p["this"][0]), H, 50.0,
                                                                  st())), o, 2.0 * M * D * D)
    del p, o
    P, frames = 18, M // 256
    v = (torch.rand((frames, 16 * P, 16 * P, 3), generator=g, device=dev) * 4 - 1).to(torch.bfloat16)
    kb = (torch.randn((P * P * 3, D), generator=g, device=dev) / (P * P * 3) ** 0.5).to(torch.bfloat16)
    wvid = nat.video_patch_w(kb.cpu(), P).to(dev)
    pos = torch.randn((256, D), generator=g, device=dev) * 0.1
    e = {k: [torch.empty(M, D, device=dev, dtype=torch.bfloat16)] for k in libs}
    ab("patch embed <6,AVID>", lambda k: _ok(libs[k].vp_dev_patch_embed(ptr(v), frames, P, ptr(wvid), D, ptr(b), ptr(pos),
                                                                       ptr(e[k][0]), st())), e, 2.0 * M * D * 64 * P)


def _ok(rc):
    assert rc == 0, nat.load().vp_last_error()


if __name__ == "__main__":
    if sys.argv[1] == "pooler":
        pooler(sys.argv[2], control=sys.argv[3:] == ["control"])
    elif sys.argv[1] == "gemm":
        gemm(sys.argv[2:])
    else:
        {"tattn": tattn, "spatial": spatial, "attention": attention}[sys.argv[1]](sys.argv[2])
