"""Child process of oracle/make_ref_fixtures.py: runs calls into the reference's own modules on the stand-ins.

    python child.py REFERENCE_ROOT MODE JOB.npz OUT.npz

The reference's package and this repository's are both called `videoprism`, so this process keeps the
repository's package off `sys.path`: it holds the reference root and the directory of `refshim`, nothing else of
the repository.  JOB.npz holds the arrays and, under `__job__`, a JSON list of calls; OUT.npz receives every
call's outputs under `<id>`, `<id>/<index>` or `<id>/<key>`.

Values in a call's `ctor`, `args` and `kwargs` are JSON, with these forms resolved here:
  {"$a": key}            the array `key` of JOB.npz (floats in the mode's float type)
  {"$attr": "mod.name"}  an attribute of a reference module (`layers.gelu`)
  {"$tuple": [...]}, {"$set": [...]}
  {"$ref": id, "at": i}  output i of an earlier call
"""

import dataclasses
import importlib
import json
import os
import sys


def _paths(ref_root):
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(os.path.dirname(here))
    keep = [p for p in sys.path if p and not os.path.abspath(p).startswith(repo)]
    sys.path[:] = [os.path.abspath(ref_root), os.path.dirname(here)] + keep


def _settings(obj, prefix=""):
    """A module's dataclass fields as {dotted name: int | float | str | bool | None | list}; nested modules and
    dicts flattened; dtypes and the parent link left out; functions by name."""
    out = {}
    items = ([(f.name, getattr(obj, f.name)) for f in dataclasses.fields(obj)] if dataclasses.is_dataclass(obj)
             else list(obj.items()))
    for k, v in items:
        if k in ("parent", "name", "dtype", "fprop_dtype"):
            continue
        key = f"{prefix}{k}"
        if dataclasses.is_dataclass(v) or isinstance(v, dict):
            out.update(_settings(v, key + "."))
        elif isinstance(v, (tuple, list)):
            out[key] = list(v)
        elif v is None or isinstance(v, (bool, int, float, str)):
            out[key] = v
        elif callable(v):
            out[key] = getattr(v, "__name__", repr(v))
        else:
            raise TypeError(f"setting {key}: {type(v)}")
    return out


def main(ref_root, mode, job_path, out_path):
    _paths(ref_root)
    import numpy as np
    import refshim
    refshim.install(mode)
    from jax import numpy as jnp
    mods = {}

    def module(name):
        if name not in mods:
            mods[name] = importlib.import_module(f"videoprism.{name}")
            origin = os.path.abspath(mods[name].__file__)
            assert origin.startswith(os.path.abspath(ref_root)), origin
        return mods[name]

    def attr(dotted):
        mod, name = dotted.split(".", 1)
        obj = module(mod)
        for part in name.split("."):
            obj = getattr(obj, part)
        return obj

    job = np.load(job_path, allow_pickle=False)
    calls = json.loads(str(job["__job__"]))
    results, out = {}, {}

    def value(v):
        if isinstance(v, dict):
            if "$a" in v:
                return jnp.asarray(job[v["$a"]])
            if "$attr" in v:
                return attr(v["$attr"])
            if "$tuple" in v:
                return tuple(value(x) for x in v["$tuple"])
            if "$set" in v:
                return {value(x) for x in v["$set"]}
            if "$ref" in v:
                r = results[v["$ref"]]
                return r if v.get("at") is None else r[v["at"]]
            return {k: value(x) for k, x in v.items()}
        if isinstance(v, list):
            return [value(x) for x in v]
        return v

    def tree(prefix):
        root = {}
        for key in job.files:
            if key.startswith(prefix):
                node = root
                parts = key[len(prefix):].split("/")
                for p in parts[:-1]:
                    node = node.setdefault(p, {})
                node[parts[-1]] = job[key]
        return {"params": root}

    def record(key, r):
        if r is None:
            return
        if isinstance(r, (tuple, list)):
            for i, x in enumerate(r):
                record(f"{key}/{i}", x)
        elif isinstance(r, dict):
            for k, x in r.items():
                record(f"{key}/{k}", x)
        else:
            out[key] = np.asarray(r)

    for c in calls:
        args = [value(a) for a in c.get("args", [])]
        kwargs = {k: value(a) for k, a in c.get("kwargs", {}).items()}
        try:
            if c["kind"] == "apply":
                m = attr(c["cls"])(**{k: value(a) for k, a in c.get("ctor", {}).items()})
                r = m.apply(tree(c["params"]) if c.get("params") else {"params": {}}, *args, **kwargs)
            elif c["kind"] == "fn":
                r = attr(c["fn"])(*args, **kwargs)
            elif c["kind"] == "builder":
                r = None
                out[c["id"] + "/settings"] = np.array(json.dumps(_settings(attr(c["fn"])(*args, **kwargs)),
                                                                 sort_keys=True))
            elif c["kind"] == "constant":
                r = None
                out[c["id"] + "/settings"] = np.array(json.dumps(attr(c["fn"]), sort_keys=True))
            else:
                raise ValueError(c["kind"])
        except Exception as e:  # noqa: BLE001 -- a call may be there to show that the program refuses it
            if not c.get("expect_error"):
                raise RuntimeError(f"call {c['id']} failed") from e
            out[c["id"] + "/raised"] = np.array(type(e).__name__)
            continue
        if c.get("expect_error"):
            out[c["id"] + "/raised"] = np.array("")
        results[c["id"]] = r
        record(c["id"], r)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(*sys.argv[1:5])
