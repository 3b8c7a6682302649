"""NumPy restatement of the colour conversion in front of the frame preprocessing: what the HIP kernel
(csrc/preprocess.hip, vp_op_preprocess_yuv) computes for each tap of a decoder's 4:2:0 planes before the
resize of tests/preprocess_restatement.py runs on the result:

    preprocess_yuv(planes) == preprocess_restatement.preprocess(yuv_to_rgb(planes)),  uint8, bit for bit.

Chroma is not interpolated: luma pixel (y, x) uses chroma sample (y >> 1, x >> 1); the chroma planes are
ceil(H/2) x ceil(W/2), so odd H and W are legal.

Formats: "nv12" (8-bit: Y [.., H, W], interleaved UV [.., ch, cw, 2]), "i420" (8-bit: Y, U [.., ch, cw], V),
"p010" (NV12's layout in 16-bit words, the d = 10-bit sample is word >> 6).

With s = 2^(d-8):  limited: yoff = 16 s, ygain = 255 / (219 s), cgain = 255 / (224 s);
                   full:    yoff = 0,    ygain = cgain = 255 / (2^d - 1);          coff = 128 s in both.
bt601: Kr = 0.299, Kb = 0.114;  bt709: Kr = 0.2126, Kb = 0.0722;  Kg = 1 - Kr - Kb.
    R = ygain (Y - yoff)                                          + cgain 2 (1 - Kr) (V - coff)
    G = ygain (Y - yoff) - cgain 2 (1 - Kb) Kb / Kg (U - coff)    - cgain 2 (1 - Kr) Kr / Kg (V - coff)
    B = ygain (Y - yoff) + cgain 2 (1 - Kb) (U - coff)
Integer form (what is computed): every coefficient is floor(x * 65536 + 0.5) as int32, and
    out = clip((cy (Y - yoff) + cu (U - coff) + cv (V - coff) + 32768) >> 16, 0, 255)
in int32 with an arithmetic shift; Y below yoff is not clamped first.  The formula is the project's own: no
parity with cv2.cvtColor is claimed.
"""

import numpy as np

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("limited", "full")
BIT_DEPTH = {"nv12": 8, "i420": 8, "p010": 10}


def real_coefficients(matrix: str, color_range: str, bit_depth: int):
    """(float64 [3, 3] rows R, G, B x (cy, cu, cv), yoff, coff) of the real-valued form."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    s = float(1 << (bit_depth - 8))
    full = float((1 << bit_depth) - 1)
    if color_range == "limited":
        yoff, ygain, cgain = 16 << (bit_depth - 8), 255.0 / (219.0 * s), 255.0 / (224.0 * s)
    elif color_range == "full":
        yoff, ygain, cgain = 0, 255.0 / full, 255.0 / full
    else:
        raise ValueError(f"Unknown color_range: {color_range}")
    m = np.array([[ygain, 0.0, cgain * 2.0 * (1.0 - kr)],
                  [ygain, -(cgain * 2.0 * (1.0 - kb) * kb / kg), -(cgain * 2.0 * (1.0 - kr) * kr / kg)],
                  [ygain, cgain * 2.0 * (1.0 - kb), 0.0]], dtype=np.float64)
    return m, yoff, 128 << (bit_depth - 8)


def coefficients(matrix: str, color_range: str, bit_depth: int):
    """(int32 [3, 3], yoff, coff) of the integer form."""
    m, yoff, coff = real_coefficients(matrix, color_range, bit_depth)
    return np.floor(m * 65536.0 + 0.5).astype(np.int32), yoff, coff


def accumulate(y, u, v, matrix: str, color_range: str, bit_depth: int):
    """The sums before the shift, int64 [..., 3], for sample arrays y, u, v of one shape (to show they fit int32)."""
    c, yoff, coff = coefficients(matrix, color_range, bit_depth)
    c = c.astype(np.int64)
    d = np.stack([np.asarray(y, np.int64) - yoff, np.asarray(u, np.int64) - coff, np.asarray(v, np.int64) - coff], -1)
    return d[..., None, 0] * c[:, 0] + d[..., None, 1] * c[:, 1] + d[..., None, 2] * c[:, 2] + 32768


def convert(y, u, v, matrix: str, color_range: str, bit_depth: int):
    """uint8 [..., 3] R, G, B of sample arrays y, u, v of one shape: the integer form, in int32."""
    c, yoff, coff = coefficients(matrix, color_range, bit_depth)
    yy = np.asarray(y).astype(np.int32) - np.int32(yoff)
    uu = np.asarray(u).astype(np.int32) - np.int32(coff)
    vv = np.asarray(v).astype(np.int32) - np.int32(coff)
    out = [(c[k, 0] * yy + c[k, 1] * uu + c[k, 2] * vv + np.int32(32768)) >> 16 for k in range(3)]
    return np.clip(np.stack(out, -1), 0, 255).astype(np.uint8)


def convert_real(y, u, v, matrix: str, color_range: str, bit_depth: int):
    """float64 [..., 3]: the real-valued form, clipped to [0, 255] and not rounded."""
    m, yoff, coff = real_coefficients(matrix, color_range, bit_depth)
    d = np.stack([np.asarray(y, np.float64) - yoff, np.asarray(u, np.float64) - coff, np.asarray(v, np.float64) - coff], -1)
    return np.clip(d @ m.T, 0.0, 255.0)


def samples(planes, pixel_format: str):
    """(Y [.., H, W], U [.., ch, cw], V [.., ch, cw]) integer sample arrays of a tuple of planes."""
    if pixel_format == "i420":
        y, u, v = planes
    elif pixel_format in ("nv12", "p010"):
        y, uv = planes
        u, v = uv[..., 0], uv[..., 1]
    else:
        raise ValueError(f"Unknown pixel_format: {pixel_format}")
    y, u, v = (np.asarray(p) for p in (y, u, v))
    if pixel_format == "p010":
        assert all(p.dtype in (np.uint16, np.int16) for p in (y, u, v))
        y, u, v = (p.view(np.uint16) >> 6 for p in (y, u, v))  # the low 6 bits are ignored
    else:
        assert y.dtype == u.dtype == v.dtype == np.uint8
    return y, u, v


def replicate_chroma(c, h: int, w: int):
    """[.., ch, cw] -> [.., h, w]: entry (y, x) is chroma sample (y >> 1, x >> 1)."""
    return c[..., np.arange(h) >> 1, :][..., np.arange(w) >> 1]


def yuv_to_rgb(planes, pixel_format: str = "nv12", matrix: str = "bt601", color_range: str = "limited"):
    """The full-resolution frame the kernel never stores: uint8 [.., H, W, 3] in R, G, B order."""
    y, u, v = samples(planes, pixel_format)
    h, w = y.shape[-2], y.shape[-1]
    assert u.shape == v.shape == y.shape[:-2] + ((h + 1) // 2, (w + 1) // 2)
    return convert(y, replicate_chroma(u, h, w), replicate_chroma(v, h, w), matrix, color_range,
                   BIT_DEPTH[pixel_format])
