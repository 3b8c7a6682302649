"""The bf16 forward off the headline shape, element for element (cases: tests/offsize_cases.py, B = 2).  Method and
margins are test_gpu_fullsize.test_production_shape_layers_vs_wbf16_oracle's: reference point the oracle in 'wbf16'
(fp64 arithmetic on the same bf16 frames and bf16-rounded parameters), yardstick the oracle's emulation of the
reference's own bf16 graph ('bf16'); the GPU must be no further from 'wbf16' than 1.25 x the emulation's max-abs and
1.0 x its mean-abs, for `embeddings` and for `spatial_features`.  Nothing in the bar comes from the code under test.

So that a localised error cannot hide behind the whole-output mean, the same two bars hold on row subsets, the mean
taken over the subset (ours against the emulation's over the same rows), the max against the emulation's whole-output
max (a maximum over at least 3.9e5 elements at every case):

  * the rows of padded frames, and the rows of valid frames;
  * the rows of the last, partial 256-row GEMM tile (row index at or past the last multiple of 256), in the spatial
    stack's row order (b t n) and in the temporal stack's (b n t).

Every measured pair is printed, with the place and both values of the worst element."""

import numpy as np
import pytest
import torch

import offsize_cases as oc
from oracle import videoprism_oracle as orc

pytestmark = pytest.mark.gpu

B = 2


def _subsets(c, N, fp):
    """name -> boolean [B, T, N] over the tokens."""
    T = c.T
    M = B * T * N
    edge = M // 256 * 256
    b, t, n = np.meshgrid(np.arange(B), np.arange(T), np.arange(N), indexing="ij")
    pad = np.zeros((B, T), bool) if fp is None else fp > 0
    pad = np.broadcast_to(pad[:, :, None], (B, T, N))
    return {"padded frames": pad, "valid frames": ~pad,
            "partial tile, spatial order": (b * T + t) * N + n >= edge,
            "partial tile, temporal order": (b * N + n) * T + t >= edge}


@pytest.mark.parametrize("c", oc.CASES, ids=oc.case_id)
def test_offsize_bf16_vs_wbf16_oracle(cuda, c):
    cfg = oc.BASE22
    oc.assert_kernels(c, cfg, True)
    m, var = oc.encoder(cfg, True)
    video = oc.clips(c, B, True, cuda, seed=2)
    fp = oc.frame_paddings(B, c.T) if c.padded else None
    emb, out = m.apply(var, video, return_intermediate=True,
                       frame_paddings=None if fp is None else torch.from_numpy(fp).to(cuda))
    host = video.float().cpu().numpy()
    ref, rout = orc.factorized_encoder(var["params"], host, cfg, "wbf16", frame_paddings=fp, return_intermediate=True)
    emu, eout = orc.factorized_encoder(var["params"], host, cfg, "bf16", frame_paddings=fp, return_intermediate=True)
    N, D = oc.patches(cfg, c.hw), cfg["model_dim"]
    subsets = _subsets(c, N, fp)
    misses = []
    for name, got, want, ref_emu in (("spatial_features", out["spatial_features"], rout["spatial_features"],
                                      eout["spatial_features"]), ("embeddings", emb, ref, emu)):
        got = got.float().cpu().numpy().astype(np.float64).reshape(B, c.T, N, D)
        want = np.asarray(want, np.float64).reshape(B, c.T, N, D)
        ref_emu = np.asarray(ref_emu, np.float64).reshape(B, c.T, N, D)
        assert np.isfinite(got).all()
        err, eerr = np.abs(got - want), np.abs(ref_emu - want)
        assert eerr.size >= 100000
        i = np.unravel_index(np.argmax(err), err.shape)
        print(f"{oc.case_id(c)} {name}: vs wbf16 max-abs {err.max():.3e} mean-abs {err.mean():.3e} (reference bf16 "
              f"emulation {eerr.max():.3e} / {eerr.mean():.3e}); worst at clip {i[0]} frame {i[1]} patch {i[2]} column "
              f"{i[3]}: gpu {got[i]:+.6e} wbf16 {want[i]:+.6e} emulation {ref_emu[i]:+.6e}")
        if err.max() > 1.25 * eerr.max() or err.mean() > eerr.mean():
            misses.append((name, "all rows", err.max(), err.mean(), eerr.max(), eerr.mean()))
        for sub, rows in subsets.items():
            if not rows.any():
                print(f"    {sub}: no rows")
                continue
            e, ee = err[rows], eerr[rows]
            j = np.argwhere(rows)[np.argmax(e.max(axis=-1))]
            print(f"    {sub} ({int(rows.sum())} rows): max-abs {e.max():.3e} mean-abs {e.mean():.3e} (emulation "
                  f"{ee.max():.3e} / {ee.mean():.3e}; whole-output max {eerr.max():.3e}); worst row clip {j[0]} frame "
                  f"{j[1]} patch {j[2]}")
            if e.max() > 1.25 * eerr.max() or e.mean() > ee.mean():
                misses.append((name, sub, e.max(), e.mean(), eerr.max(), ee.mean()))
    assert not misses, misses
