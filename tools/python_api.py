"""The Python binding's public surface as data: tests/golden/python_api.json.

    python tools/python_api.py                  # write the fixture from this checkout
    python tools/python_api.py --check          # compare this checkout with the fixture (exit 1 and a diff on a mismatch)
    python tools/python_api.py --root DIR --check   # the same for the package of another checkout

One record for every name of the package namespace that is neither a dunder, a module nor underscore-prefixed, plus
the private names the tests use (PRIVATE_USED): functions by signature and docstring hash, classes by their function
members and properties, ctypes structures by size and field offsets, SIGNATURES by type names, constants by repr.  The
checkout's own path is written as <root>, so two checkouts of one surface give one file.  Needs no GPU and no built
library: nothing here calls lib().  Regenerate the fixture in the commit that changes the surface, never to make
tests/test_python_api.py pass after a refactor.
"""
import argparse
import ctypes
import difflib
import hashlib
import importlib
import importlib.util
import inspect
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "python_api.json")
PRIVATE_USED = ("_as_camera", "_scene_ptr", "_check", "_ao_default_directions")  # what tests/ reaches for by name


def load(root, by_directory_name=False):
    """The package of the checkout at `root`: under the name cuda_raytracing_amd from a spec (as tests/rt_testlib.py
    and __graft_entry__.py load it), or by its directory name with `root` on sys.path (as tests/test_abi.py's child
    and tools/bigleaf_cull.py do)."""
    if by_directory_name:
        sys.path.insert(0, root)
        return importlib.import_module("cuda-raytracing_amd")
    if "cuda_raytracing_amd" in sys.modules:
        return sys.modules["cuda_raytracing_amd"]
    pkg = os.path.join(root, "cuda-raytracing_amd")
    spec = importlib.util.spec_from_file_location("cuda_raytracing_amd", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["cuda_raytracing_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def _function(f):
    doc = inspect.getdoc(f)
    return {"signature": str(inspect.signature(f)), "doc_sha256": hashlib.sha256(doc.encode()).hexdigest() if doc else None}


def _type_name(t):
    return None if t is None else t.__name__


def _record(value):
    if isinstance(value, type) and issubclass(value, ctypes.Structure):
        return {"kind": "struct", "sizeof": ctypes.sizeof(value),
                "fields": [[n, _type_name(t), getattr(value, n).offset] for n, t in value._fields_]}
    if isinstance(value, type):
        members, properties = {}, []
        for name, m in vars(value).items():
            if isinstance(m, (staticmethod, classmethod)):
                m = m.__func__
            if isinstance(m, types.FunctionType):
                members[name] = _function(m)
            elif isinstance(m, property):
                properties.append(name)
        return {"kind": "class", "bases": [b.__name__ for b in value.__bases__], "members": members,
                "properties": sorted(properties)}
    if isinstance(value, types.FunctionType):
        return {"kind": "function", **_function(value)}
    if isinstance(value, (int, float, str, tuple, dict)):
        return {"kind": "constant", "repr": repr(value)}
    raise TypeError(f"no record for a {type(value).__name__}")


def describe(rt):
    """{name: record} of the loaded package `rt`."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(rt.__file__)))
    out = {}
    for name, value in vars(rt).items():
        if isinstance(value, types.ModuleType) or (name.startswith("_") and name not in PRIVATE_USED):
            continue
        if name == "SIGNATURES":
            out[name] = {"kind": "signatures",
                         "symbols": {s: [_type_name(res), [_type_name(a) for a in args]] for s, (res, args) in value.items()}}
        else:
            out[name] = _record(value)
    missing = [n for n in PRIVATE_USED if n not in out]
    assert not missing, missing
    return json.loads(json.dumps(out).replace(json.dumps(root)[1:-1], "<root>"))


def dumps(api):
    return json.dumps(api, indent=1, sort_keys=True) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is described (default: this one)")
    ap.add_argument("--by-directory-name", action="store_true", help="import the package as 'cuda-raytracing_amd' from sys.path")
    ap.add_argument("--check", action="store_true", help="compare with the fixture instead of writing it")
    ap.add_argument("-o", "--output", default=FIXTURE)
    args = ap.parse_args()
    text = dumps(describe(load(os.path.abspath(args.root), args.by_directory_name)))
    if not args.check:
        with open(args.output, "w") as f:
            f.write(text)
        print(f"{args.output}: {len(text)} bytes")
        return 0
    want = open(args.output).read()
    if text == want:
        print(f"{args.output}: reproduced bit for bit ({len(text)} bytes)")
        return 0
    sys.stdout.writelines(difflib.unified_diff(want.splitlines(True), text.splitlines(True), "fixture", "live", n=2))
    return 1


if __name__ == "__main__":
    sys.exit(main())
