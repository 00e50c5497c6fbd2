"""Generate tests/golden/user_scenes.json from the CPU oracle (oracle/rt_oracle.c): for every case of
tests/scene_cases.py, a SHA-256 per row of each oracle frame and one of the final RNG states.

tests/test_user_scenes_cpu.py asserts that the live oracle reproduces them, so a change that moves one bit of the
oracle's frames of a caller-built scene shows without a GPU (and says in which rows).
Run from the repo root after building: python tools/make_user_scenes_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_cases as C  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(case):
    o = C.oracle_frames(case)
    return {"size": [case["width"], case["height"]], "spp": case["spp"], "bounces": case["bounces"],
            "rows": [[sha(row) for row in f] for f in o["frames"]], "rng": sha(o["rng"])}


def main():
    g = {c["name"]: digest(c) for c in C.CASES}
    path = os.path.join(ROOT, "tests", "golden", "user_scenes.json")
    with open(path, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(g)} cases")


if __name__ == "__main__":
    main()
