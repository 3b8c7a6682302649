"""The array type of the stand-ins: an immutable-by-convention ndarray subclass.

jax arrays cannot be written to: `x += y` rebinds `x` to a new array.  On a plain ndarray the same
statement writes into `x`, and with it into whatever `x` is a view of -- a caller's paddings, a
parameter leaf.  `Arr` makes every augmented assignment out of place, and funnels every ufunc result
through `wrap`, which in native mode also narrows float64 to float32 the way jax without x64 does.
"""

import numpy as np

MODE = None   # set by refshim.install


def float_dtype():
    return np.float64 if MODE == "wide" else np.float32


def wrap(x):
    """ndarray / NumPy scalar -> Arr (narrowed in native mode); tuples and lists elementwise; the rest as is."""
    if isinstance(x, (tuple, list)):
        return type(x)(wrap(v) for v in x)
    if isinstance(x, (np.ndarray, np.generic)):
        a = np.asarray(x)
        if MODE == "native":
            if a.dtype == np.float64:
                a = a.astype(np.float32)
            elif a.dtype == np.int64:
                a = a.astype(np.int32)
        return a.view(Arr)
    return x


def unwrap(x):
    if isinstance(x, Arr):
        return x.view(np.ndarray)
    if isinstance(x, (tuple, list)):
        return type(x)(unwrap(v) for v in x)
    return x


class Arr(np.ndarray):
    __array_priority__ = 100.0

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kwargs):
        if out is not None and any(o is not None for o in (out if isinstance(out, tuple) else (out,))):
            raise TypeError("arrays of the stand-in jax are immutable: no out= argument")
        res = getattr(ufunc, method)(*[unwrap(i) for i in inputs], **kwargs)
        return wrap(res)

    def _out_of_place(op):
        def f(self, other):
            return getattr(self, op)(other)
        return f

    __iadd__ = _out_of_place("__add__")
    __isub__ = _out_of_place("__sub__")
    __imul__ = _out_of_place("__mul__")
    __itruediv__ = _out_of_place("__truediv__")
    __ifloordiv__ = _out_of_place("__floordiv__")
    __ipow__ = _out_of_place("__pow__")
    __imatmul__ = _out_of_place("__matmul__")
    del _out_of_place

    def __setitem__(self, key, value):
        raise TypeError("arrays of the stand-in jax are immutable: use .at[] in jax, nothing here")

    def astype(self, dtype, *args, **kwargs):
        return wrap(self.view(np.ndarray).astype(dtype, *args, **kwargs))
