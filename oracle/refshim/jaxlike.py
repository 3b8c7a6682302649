"""Stand-in `jax`: numpy, nn, lax, image, tree, tree_util, typing, checkpoint_policies, jit, Array."""

import types
import typing

import numpy as np
from scipy import special as _sp

from . import arrays
from .arrays import Arr, unwrap, wrap


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    return m


def _dtype(dt):
    """A dtype argument as the stand-in understands it: float kinds follow the mode."""
    if dt is None:
        return None
    d = np.dtype(dt)
    if d.kind == "f":
        return np.dtype(arrays.float_dtype())
    if arrays.MODE == "native" and d == np.int64:
        return np.dtype(np.int32)
    return d


def _axis(axis):
    return tuple(axis) if isinstance(axis, list) else axis


def _lift(fn):
    """A NumPy function on plain ndarrays, returning stand-in arrays."""
    def f(*args, **kwargs):
        if "axis" in kwargs:
            kwargs["axis"] = _axis(kwargs["axis"])
        if "dtype" in kwargs:
            kwargs["dtype"] = _dtype(kwargs["dtype"])
        return wrap(fn(*[unwrap(a) for a in args], **{k: unwrap(v) for k, v in kwargs.items()}))
    f.__name__ = getattr(fn, "__name__", "lifted")
    return f


# name-for-name NumPy
_PLAIN = ("mean", "sum", "square", "sqrt", "tanh", "exp", "sin", "cos", "where", "minimum", "maximum", "multiply",
          "einsum", "tile", "transpose", "reshape", "squeeze", "expand_dims", "concatenate", "pad", "repeat")


def _bfloat16_native(*_a, **_k):
    raise NotImplementedError("bfloat16 dtype flow is not emulated by the stand-in jax (native mode)")


def _build_numpy():
    fd = arrays.float_dtype()
    jnp = _module("jax.numpy")
    for name in _PLAIN:
        setattr(jnp, name, _lift(getattr(np, name)))
    jnp.float32 = fd
    jnp.float64 = fd
    jnp.bfloat16 = fd if arrays.MODE == "wide" else _bfloat16_native
    jnp.int32 = np.int32
    jnp.dtype = np.dtype
    jnp.inexact, jnp.floating, jnp.integer = np.inexact, np.floating, np.integer
    jnp.issubdtype = np.issubdtype
    jnp.finfo, jnp.iinfo = np.finfo, np.iinfo
    jnp.newaxis = None
    jnp.nan = np.nan

    def asarray(x, dtype=None):
        a = np.asarray(unwrap(x))
        dt = _dtype(dtype) if dtype is not None else (_dtype(a.dtype) if a.dtype.kind == "f" else None)
        return wrap(a.astype(dt) if dt is not None and a.dtype != dt else a)

    def arange(*args, dtype=None):
        return wrap(np.arange(*args, dtype=_dtype(dtype)))

    def zeros(shape, dtype=None):
        return wrap(np.zeros(tuple(shape) if not np.isscalar(shape) else shape, dtype=_dtype(dtype or fd)))

    jnp.asarray = asarray
    jnp.array = asarray
    jnp.arange = arange
    jnp.zeros = zeros
    return jnp


# ---- jax.nn ----

def _softmax(x, axis=-1):
    x = unwrap(x)
    e = np.exp(x - np.max(x, axis=axis, keepdims=True))
    return wrap(e / np.sum(e, axis=axis, keepdims=True))


def _gelu(x, approximate=True):
    x = unwrap(x)
    if approximate:
        raise NotImplementedError("gelu: the exact (erf) form only")
    return wrap((0.5 * x * _sp.erfc(-x * np.sqrt(0.5))).astype(x.dtype))


def _one_hot(x, num_classes, dtype=None, axis=-1):
    if axis != -1:
        raise NotImplementedError("one_hot: last axis only")
    x = unwrap(x)
    return wrap((x[..., None] == np.arange(num_classes)).astype(_dtype(dtype or arrays.float_dtype())))


def _relu(x):
    x = unwrap(x)
    return wrap(np.maximum(x, np.zeros((), x.dtype)))


def _softplus(x):
    x = unwrap(x)
    return wrap(np.logaddexp(x, np.zeros((), x.dtype)))


# ---- jax.lax ----

def _rsqrt(x):
    x = unwrap(x)
    return wrap(np.ones((), x.dtype) / np.sqrt(x))


def _slice_in_dim(operand, start_index, limit_index, stride=1, axis=0):
    x = unwrap(operand)
    n = x.shape[axis]
    start = 0 if start_index is None else int(start_index)
    limit = n if limit_index is None else int(limit_index)
    # lax.slice takes no out-of-range bounds: it raises where a Python slice would clip
    if not (0 <= start <= limit <= n):
        raise TypeError(f"slice_in_dim: bounds [{start}, {limit}) outside a dimension of size {n}")
    idx = [slice(None)] * x.ndim
    idx[axis] = slice(start, limit, stride)
    return wrap(x[tuple(idx)])


# ---- jax.image ----

def resize_weights(in_size, out_size, antialias=True):
    """The [out, in] weights of jax.image.resize(method='linear' / 'bilinear') along one dimension, as
    scale_and_translate with scale = out / in and no translation defines them: output pixel o samples the input
    at the half-pixel centre (o + 0.5) * in / out - 0.5 with a triangle kernel of radius max(1, in / out) (the
    widening is the antialiasing, so it applies only when shrinking); the taps that fall on input pixels are
    renormalised to sum 1, so at an edge the out-of-range part of the kernel is dropped, not clamped."""
    scale = out_size / in_size
    radius = max(1.0 / scale, 1.0) if antialias else 1.0
    w = np.zeros((out_size, in_size), np.float64)
    for o in range(out_size):
        centre = (o + 0.5) / scale - 0.5
        if centre < -0.5 or centre > in_size - 0.5:
            continue                               # a sample outside the image contributes nothing
        for i in range(in_size):
            w[o, i] = max(0.0, 1.0 - abs(centre - i) / radius)
        total = w[o].sum()
        w[o] = w[o] / total if abs(total) > 1000.0 * np.finfo(np.float32).eps else 0.0
    return w


def _resize(image, shape, method, antialias=True, precision=None):
    if method != "bilinear":
        raise NotImplementedError(f"resize: method {method!r}")
    x = unwrap(image)
    shape = tuple(int(s) for s in shape)
    if len(shape) != x.ndim:
        raise ValueError("resize: shape must have the rank of the image")
    out = x
    for d, (n_in, n_out) in enumerate(zip(x.shape, shape)):
        if n_in == n_out:
            continue
        w = resize_weights(n_in, n_out, antialias).astype(x.dtype if x.dtype.kind == "f" else np.float64)
        out = np.moveaxis(np.tensordot(w, out, axes=([1], [d])), 0, d)
    return wrap(out.astype(x.dtype) if x.dtype.kind == "f" else out)


# ---- pytrees: dicts (keys sorted), lists, tuples; None is an empty subtree ----

def _tree_map(f, tree, *rest, is_leaf=None):
    if is_leaf is not None and is_leaf(tree):
        return f(tree, *rest)
    if tree is None:
        return None
    if isinstance(tree, dict):
        return {k: _tree_map(f, tree[k], *[r[k] for r in rest], is_leaf=is_leaf) for k in sorted(tree)}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_tree_map(f, v, *[r[i] for r in rest], is_leaf=is_leaf) for i, v in enumerate(tree))
    return f(tree, *rest)


class _TreeDef:
    def __init__(self, skeleton, n):
        self.skeleton, self.num_leaves = skeleton, n

    def unflatten(self, leaves):
        it = iter(leaves)
        return _tree_map(lambda _: next(it), self.skeleton)


def _tree_flatten(tree, is_leaf=None):
    leaves = []
    skeleton = _tree_map(lambda x: (leaves.append(x), 0)[1], tree, is_leaf=is_leaf)
    return leaves, _TreeDef(skeleton, len(leaves))


def build():
    jnp = _build_numpy()
    nn = _module("jax.nn", softmax=_softmax, gelu=_gelu, one_hot=_one_hot, relu=_relu, softplus=_softplus)
    lax = _module("jax.lax", rsqrt=_rsqrt, slice_in_dim=_slice_in_dim)
    image = _module("jax.image", resize=_resize)
    tree = _module("jax.tree", map=_tree_map, flatten=_tree_flatten)
    tree_util = _module("jax.tree_util", tree_map=_tree_map, tree_flatten=_tree_flatten)
    typing_ = _module("jax.typing", DTypeLike=typing.Any)
    policies = _module("jax.checkpoint_policies", nothing_saveable=None)
    jax = _module("jax", numpy=jnp, nn=nn, lax=lax, image=image, tree=tree, tree_util=tree_util, typing=typing_,
                  checkpoint_policies=policies, Array=Arr, jit=lambda f, *a, **k: f)
    jax.__path__ = []          # a package, so that `from jax import numpy` and `import jax.numpy` both resolve
    return {"jax": jax, "jax.numpy": jnp, "jax.nn": nn, "jax.lax": lax, "jax.image": image, "jax.tree": tree,
            "jax.tree_util": tree_util, "jax.typing": typing_, "jax.checkpoint_policies": policies}
