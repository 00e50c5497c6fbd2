"""The package's public surface against tests/golden/python_api.json (tools/python_api.py writes it): every public
name, signature, docstring, structure layout, library signature and constant, exactly and in both directions, under
both names the package is loaded by.  No GPU and no built library."""
import importlib.util
import json
import os
import subprocess
import sys

import rt_testlib as T

TOOL = os.path.join(T.ROOT, "tools", "python_api.py")
FIXTURE = os.path.join(T.GOLDEN, "python_api.json")


def tool():
    spec = importlib.util.spec_from_file_location("rt_python_api", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_surface_loaded_as_cuda_raytracing_amd():
    api = tool()
    live, want = api.describe(T.load_rt()), json.load(open(FIXTURE))
    assert sorted(set(want) - set(live)) == [], "names that left the package"
    assert sorted(set(live) - set(want)) == [], "names that leaked into the package (regenerate the fixture with the new name)"
    changed = {k: (want[k], live[k]) for k in want if want[k] != live[k]}
    assert not changed, changed
    assert api.dumps(live) == open(FIXTURE).read()


def test_surface_imported_by_directory_name():
    """importlib.import_module("cuda-raytracing_amd") with the repository root on sys.path, in a child process of its
    own: the package is then not known as cuda_raytracing_amd at all."""
    r = subprocess.run([sys.executable, TOOL, "--by-directory-name", "--check"], capture_output=True, text=True, timeout=120,
                       cwd=T.ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "reproduced bit for bit" in r.stdout
