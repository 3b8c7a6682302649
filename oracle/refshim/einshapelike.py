"""Stand-in `einshape`: `jax_einshape(equation, x, **sizes)`.

An einshape equation is `lhs->rhs` over one-letter axis names; parentheses group axes that share one dimension
(`(bt)nd->(bn)td`).  Sizes of grouped axes come from the keyword arguments; at most one axis per group may be left
to be inferred.  The result is reshape (ungroup) -> transpose -> reshape (regroup).
"""

import types

import numpy as np

from .arrays import unwrap, wrap


def _parse(side):
    groups, i = [], 0
    while i < len(side):
        c = side[i]
        if c == "(":
            j = side.index(")", i)
            groups.append(list(side[i + 1:j]))
            i = j + 1
        elif c.isalpha():
            groups.append([c])
            i += 1
        elif c.isspace():
            i += 1
        else:
            raise ValueError(f"einshape: cannot parse {side!r}")
    return groups


def einshape(equation, x, **sizes):
    x = unwrap(x)
    lhs, rhs = equation.replace(" ", "").split("->")
    lg, rg = _parse(lhs), _parse(rhs)
    if len(lg) != x.ndim:
        raise ValueError(f"einshape: {lhs!r} has {len(lg)} dimensions, the array {x.ndim}")
    names = [n for g in lg for n in g]
    if sorted(names) != sorted(n for g in rg for n in g) or len(set(names)) != len(names):
        raise ValueError(f"einshape: {equation!r} must name every axis once on each side")
    size = dict(sizes)
    for g, dim in zip(lg, x.shape):
        unknown = [n for n in g if n not in size]
        known = int(np.prod([size[n] for n in g if n in size], dtype=np.int64))
        if len(unknown) > 1:
            raise ValueError(f"einshape: sizes of {unknown} cannot both be inferred")
        if unknown:
            if dim % known:
                raise ValueError(f"einshape: dimension {dim} is not divisible by {known}")
            size[unknown[0]] = dim // known
        elif known != dim:
            raise ValueError(f"einshape: group {g} has size {known}, the array {dim}")
    y = x.reshape([size[n] for n in names])
    y = y.transpose([names.index(n) for g in rg for n in g])
    return wrap(y.reshape([int(np.prod([size[n] for n in g], dtype=np.int64)) for g in rg]))


def build():
    m = types.ModuleType("einshape")
    m.jax_einshape = einshape
    return {"einshape": m}
