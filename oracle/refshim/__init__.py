"""NumPy stand-ins for the third-party modules the reference's Flax program imports.

TEST INFRASTRUCTURE ONLY.  `install(mode)` builds stand-in modules named `jax` (with `jax.numpy`,
`jax.nn`, `jax.lax`, `jax.image`, `jax.tree`, `jax.tree_util`, `jax.typing`), `flax` / `flax.linen`
and `einshape`, and puts them into `sys.modules`, so that the reference's own `layers.py`,
`encoders.py`, `models.py` and `utils.py` can be imported and executed on a NumPy backend.  Nothing
happens on import of this package: no file here is called `jax.py` or `flax.py`, none sits on
`sys.path` under those names, and `install` refuses to shadow a real jax or flax.

Written from the public API semantics of jax, flax.linen and einshape; it covers what the reference's
four files touch and no more, and is apply-only (no initialisation, no gradients, no PRNG).

Two numeric modes:
  wide    `jnp.float32`, `jnp.bfloat16` and `jnp.float64` are all NumPy float64, so every parameter,
          every `astype` and every constant of the program is float64: the reference's graph in fp64.
  native  `jnp.float32` is float32 and, as in jax without x64, no result is ever float64.
bf16 dtype flow is not emulated in either mode (no bfloat16 NumPy dtype is available): in native mode
`jnp.bfloat16` raises.
"""

import sys

MODES = ("wide", "native")
_NAMES = ("jax", "jax.numpy", "jax.nn", "jax.lax", "jax.image", "jax.tree", "jax.tree_util",
          "jax.typing", "jax.checkpoint_policies", "flax", "flax.linen", "flax.linen.module",
          "flax.linen.initializers", "einshape")


def install(mode="wide"):
    """Put the stand-ins into sys.modules; returns {name: module}.  One mode per process."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    for name in _NAMES:
        mod = sys.modules.get(name)
        if mod is not None and not getattr(mod, "__refshim__", False):
            raise RuntimeError(f"a real {name!r} is already imported; the stand-ins never shadow it")
    from . import arrays, einshapelike, flaxlike, jaxlike
    if arrays.MODE is not None and arrays.MODE != mode:
        raise RuntimeError(f"stand-ins already installed in mode {arrays.MODE!r}")
    arrays.MODE = mode
    mods = {}
    mods.update(jaxlike.build())
    mods.update(flaxlike.build(mods["jax"]))
    mods.update(einshapelike.build())
    for name, mod in mods.items():
        mod.__refshim__ = True
        sys.modules[name] = mod
    return mods


def uninstall():
    """Remove the stand-ins again (used by the self-tests, which install them in-process)."""
    from . import arrays
    for name in _NAMES:
        mod = sys.modules.get(name)
        if mod is not None and getattr(mod, "__refshim__", False):
            del sys.modules[name]
    arrays.MODE = None
