"""Stand-in `flax.linen`, apply-only.

A module is a dataclass of its annotated fields plus keyword-only `name` and `parent`.  A module built while
another module's `@compact` method (or `apply`) runs becomes that module's child; its scope path is its parent's
path plus its `name` (or `<Class>_<n>` when unnamed).  `self.param(name, init, shape, dtype)` looks the leaf up by
scope path in the `{'params': tree}` handed to `apply`; it raises on a missing leaf and on a shape mismatch, and
`apply` raises when it returns with a leaf the program never read.  Initialisers are inert.

`scan(fn, variable_axes={'params': 0}, length=n)(module, carry)` runs `fn(module, carry)` n times in a Python
loop; in pass i every leaf under the module's scope is read as `leaf[i]`.  `remat` is the identity.
"""

import dataclasses
import functools
import types
import typing

import numpy as np

from . import arrays
from .arrays import wrap


class _Store:
    def __init__(self, variables):
        if not isinstance(variables, dict) or "params" not in variables:
            raise ValueError("apply needs {'params': tree}")
        self.leaves = {}
        self._walk(variables["params"], ())
        self.read = set()
        self.slices = []          # (scope path, index) of the scans in progress, outermost first

    def _walk(self, tree, path):
        for k, v in tree.items():
            if isinstance(v, dict):
                self._walk(v, path + (str(k),))
            else:
                self.leaves[path + (str(k),)] = v

    def get(self, path, shape):
        name = "/".join(path)
        if path not in self.leaves:
            raise KeyError(f"no parameter {name!r} in the supplied tree")
        leaf = np.asarray(self.leaves[path])
        for scope, i in self.slices:
            if path[:len(scope)] == scope:
                leaf = leaf[i]
        if tuple(leaf.shape) != tuple(int(s) for s in shape):
            raise ValueError(f"parameter {name!r}: the program asks for shape {tuple(shape)}, the tree holds "
                             f"{tuple(leaf.shape)}")
        self.read.add(path)
        return leaf

    def unread(self):
        return sorted("/".join(p) for p in set(self.leaves) - self.read)


_STACK = []      # modules whose compact method (or apply) is running, innermost last
_STORE = []      # the parameter store of the apply in progress


def compact(fn):
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        _STACK.append(self)
        try:
            return fn(self, *args, **kwargs)
        finally:
            _STACK.pop()
    wrapped.__compact__ = True
    return wrapped


def nowrap(fn):
    return fn


class Module:
    name = None
    parent = None

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        ann = {k: v for k, v in cls.__dict__.get("__annotations__", {}).items() if k not in ("name", "parent")}
        ann["_refshim_kw_only"] = dataclasses.KW_ONLY
        ann["name"] = typing.Optional[str]
        ann["parent"] = typing.Any
        cls.__annotations__ = ann
        cls.name = None
        cls.parent = None
        dataclasses.dataclass(cls, eq=False, repr=False)

    def __post_init__(self):
        if self.parent is None and _STACK:
            object.__setattr__(self, "parent", _STACK[-1])
        if self.parent is not None and self.name is None:
            counts = self.parent.__dict__.setdefault("_refshim_autonames", {})
            n = counts.get(type(self).__name__, 0)
            counts[type(self).__name__] = n + 1
            object.__setattr__(self, "name", f"{type(self).__name__}_{n}")

    @property
    def path(self):
        if self.parent is None:
            return ()
        return self.parent.path + (self.name,)

    def param(self, name, init_fn, *init_args, **_unused):
        if not _STORE:
            raise RuntimeError("param() outside apply(): the stand-in flax is apply-only")
        shape = init_args[0] if init_args else ()
        dtype = init_args[1] if len(init_args) > 1 else None
        leaf = _STORE[-1].get(self.path + (name,), shape)
        if leaf.dtype.kind == "f" or dtype is not None:
            leaf = leaf.astype(arrays.float_dtype())
        return wrap(np.array(leaf))

    def apply(self, variables, *args, method=None, rngs=None, mutable=False, **kwargs):
        if mutable:
            raise NotImplementedError("apply(mutable=...) is not part of the stand-in")
        if self.parent is not None:
            raise RuntimeError("apply() on a bound submodule")
        store = _Store(variables)
        self.__dict__.pop("_refshim_autonames", None)
        _STORE.append(store)
        _STACK.append(self)
        try:
            fn = self.__call__ if method is None else (getattr(self, method) if isinstance(method, str)
                                                       else functools.partial(method, self))
            out = fn(*args, **kwargs)
        finally:
            _STACK.pop()
            _STORE.pop()
        unread = store.unread()
        if unread:
            raise ValueError(f"{len(unread)} parameter(s) of the supplied tree were never read: {unread[:6]}")
        return out


def _inert(kind):
    def factory(*_args, **_kwargs):
        def init(*_a, **_k):
            raise RuntimeError(f"initialiser {kind} called: the stand-in flax is apply-only")
        init.__name__ = kind
        return init
    return factory


def _default_promote(*args, dtype=None, inexact=True):
    return args


class Dense(Module):
    features: int
    use_bias: bool = True
    dtype: typing.Any = None
    param_dtype: typing.Any = None
    precision: typing.Any = None
    kernel_init: typing.Any = None
    bias_init: typing.Any = None
    promote_dtype: typing.Any = _default_promote

    @compact
    def __call__(self, inputs):
        kernel = self.param("kernel", self.kernel_init, (inputs.shape[-1], self.features), self.param_dtype)
        bias = self.param("bias", self.bias_init, (self.features,), self.param_dtype) if self.use_bias else None
        inputs, kernel, bias = self.promote_dtype(inputs, kernel, bias, dtype=self.dtype)
        y = wrap(np.matmul(np.asarray(inputs), np.asarray(kernel)))
        if bias is not None:
            y = y + bias.reshape((1,) * (y.ndim - 1) + (-1,))
        return y


class Dropout(Module):
    rate: float
    broadcast_dims: typing.Any = ()
    deterministic: typing.Optional[bool] = None
    rng_collection: str = "dropout"

    def __call__(self, inputs, deterministic=None, rng=None):
        det = self.deterministic if deterministic is None else deterministic
        if det or self.rate == 0.0:
            return inputs
        raise NotImplementedError("Dropout with deterministic=False: the stand-in flax has no PRNG")


def remat(fn, *_args, **_kwargs):
    return fn


def scan(fn, variable_axes=None, split_rngs=None, length=None, **unsupported):
    if dict(variable_axes or {}) != {"params": 0}:
        raise NotImplementedError("scan: variable_axes={'params': 0} only")
    if length is None or unsupported.get("in_axes", 0) != 0 or unsupported.get("out_axes", 0) != 0:
        raise NotImplementedError("scan: a fixed length and the default in/out axes only")

    def scanned(module, carry, *xs):
        if xs:
            raise NotImplementedError("scan: no scanned-over inputs")
        if not _STORE:
            raise RuntimeError("scan outside apply()")
        ys = []
        for i in range(length):
            _STORE[-1].slices.append((module.path, i))
            try:
                carry, y = fn(module, carry)
            finally:
                _STORE[-1].slices.pop()
            ys.append(y)
        return carry, (None if all(y is None for y in ys) else ys)
    return scanned


def build(jax):
    init = types.ModuleType("flax.linen.initializers")
    init.Initializer = typing.Callable[..., typing.Any]
    for kind in ("lecun_normal", "constant", "zeros_init", "normal"):
        setattr(init, kind, _inert(kind))
    module = types.ModuleType("flax.linen.module")
    module.VariableDict = typing.Mapping[str, typing.Any]
    module.Module = Module
    module.compact, module.nowrap = compact, nowrap
    linen = types.ModuleType("flax.linen")
    linen.__path__ = []
    linen.__dict__.update(Module=Module, compact=compact, nowrap=nowrap, Dense=Dense, Dropout=Dropout, remat=remat,
                          scan=scan, initializers=init, module=module, relu=jax.nn.relu)
    flax = types.ModuleType("flax")
    flax.__path__ = []
    flax.linen = linen
    return {"flax": flax, "flax.linen": linen, "flax.linen.module": module, "flax.linen.initializers": init}
