"""Test helpers: load the product package and the CPU oracle (oracle/liboracle.so).

The oracle is test infrastructure (see oracle/rt_oracle.c header): it is loaded only here,
by __graft_entry__.smoke() and by bench.py's cpu_baseline leg.
"""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORACLE_LIB = os.path.join(ROOT, "oracle", "liboracle.so")
SEED = 0xDEADBEEF


def load_rt():
    if "cuda_raytracing_amd" in sys.modules:
        return sys.modules["cuda_raytracing_amd"]
    spec = importlib.util.spec_from_file_location(
        "cuda_raytracing_amd", os.path.join(ROOT, "cuda-raytracing_amd", "__init__.py"),
        submodule_search_locations=[os.path.join(ROOT, "cuda-raytracing_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["cuda_raytracing_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def header_layout(text, name):
    """(size, {field: offset}, [declared fields]) of a struct of include/rt_abi.h (`text`): the size and the offsets
    its static_assert pins (None and {} where it has none), the field names in declaration order; an array counts as
    one field."""
    size = re.search(r"sizeof\(%s\) == (\d+)" % name, text)
    offsets = dict((k, int(v)) for k, v in re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % name, text))
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        decl = re.sub(r"\[\d+\]", "", decl.strip().replace("*", " "))
        declared += re.findall(r"(\w+)\s*(?:,|$)", decl)
    return (int(size.group(1)) if size else None), offsets, declared


_P, _SZ, _I, _U32, _U64, _F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        if not os.path.exists(ORACLE_LIB):
            raise RuntimeError("oracle/liboracle.so not built (run __graft_entry__.build())")
        L = ctypes.CDLL(ORACLE_LIB)
        L.oracle_scene_create.restype = _P
        L.oracle_scene_create.argtypes = [_I, ctypes.c_char_p, _I]
        L.oracle_scene_destroy.argtypes = [_P]
        L.oracle_scene_arrays.argtypes = [_P] + [ctypes.POINTER(t) for t in (_P, _SZ, _P, _SZ, _P, _SZ, _P, _I, _P, _I, _P, _I)]
        L.oracle_camera.argtypes = [_P, _I, _I, ctypes.POINTER(_F)]
        L.oracle_set_camera.argtypes = [_P, ctypes.POINTER(_F), _F, _F]
        L.oracle_rng_init.argtypes = [_U32, _U64, ctypes.POINTER(_U32)]
        L.oracle_rng_init_frame.argtypes = [_U32, _I, _I, _P, _I]
        L.oracle_rng_draws.argtypes = [ctypes.POINTER(_U32), _I, ctypes.POINTER(_F)]
        L.oracle_jump_matrix.argtypes = [_I, ctypes.POINTER(_U32)]
        L.oracle_jump_matrix.restype = _I
        L.oracle_sin.argtypes = L.oracle_cos.argtypes = [_F]
        L.oracle_sin.restype = L.oracle_cos.restype = _F
        L.oracle_render.restype = _I
        L.oracle_render.argtypes = [_P, _I, _I, _I, _I, _I, _U32, _P, _P, _P, _I, _I, _I, _P]
        # the scene builder (rt_oracle.c "Scene builder for tests") and the per-pixel pending-entry maximum
        _FP = ctypes.POINTER(_F)
        L.oracle_scene_new.restype = _P
        L.oracle_scene_new.argtypes = []
        L.oracle_scene_add_material.argtypes = [_P, _FP]
        L.oracle_scene_add_triangle.argtypes = [_P, _FP, _FP, _FP, _I]
        L.oracle_scene_add_quad.argtypes = [_P, _FP, _FP, _FP, _FP, _I]
        L.oracle_scene_add_sphere.argtypes = [_P, _FP, _F, _I]
        L.oracle_scene_set_sky.argtypes = [_P, ctypes.c_char_p]
        L.oracle_scene_finish.argtypes = [_P]
        L.oracle_max_depth_limit.argtypes = []
        for f in (L.oracle_scene_add_material, L.oracle_scene_add_triangle, L.oracle_scene_add_quad, L.oracle_scene_add_sphere,
                  L.oracle_scene_set_sky, L.oracle_scene_finish, L.oracle_max_depth_limit, L.oracle_render_pending):
            f.restype = _I
        L.oracle_render_pending.argtypes = [_P, _I, _I, _I, _I, _I, _U32, _P, _P, _P, _I, _I, _I, _P, _P]
        _oracle = L
    return _oracle


class OracleScene:
    WHICH = {"bunny": 0, "bunny4": 1, "plane1m": 2}

    def __init__(self, which="bunny", grid_n=708):
        self.h = (oracle().oracle_scene_new() if which is None else
                  oracle().oracle_scene_create(self.WHICH[which], ASSETS.encode(), grid_n))
        if not self.h:
            raise RuntimeError("oracle_scene_create failed")

    # --- the builder: an empty scene (which=None), filled call by call, then finish() ---------------------
    @staticmethod
    def _f(v, n=3):
        v = [float(x) for x in v]
        assert len(v) == n
        return (ctypes.c_float * n)(*v)

    def add_material(self, fields16):
        """The 16 floats of a GPUMaterial, every one as given; returns its index."""
        i = oracle().oracle_scene_add_material(self.h, self._f(fields16, 16))
        assert i >= 0, "oracle material table full"
        return i

    def add_triangle(self, a, b, c, material):
        assert oracle().oracle_scene_add_triangle(self.h, self._f(a), self._f(b), self._f(c), material) == 0

    def add_quad(self, a, b, c, d, material):
        assert oracle().oracle_scene_add_quad(self.h, self._f(a), self._f(b), self._f(c), self._f(d), material) == 0

    def add_sphere(self, position, radius, material):
        assert oracle().oracle_scene_add_sphere(self.h, self._f(position), float(radius), material) == 0, "oracle sphere table full"

    def set_sky(self, path):
        assert oracle().oracle_scene_set_sky(self.h, path.encode() if path else None) == 0, f"cannot load sky {path}"

    def set_camera(self, position, angle_x, angle_y):
        oracle().oracle_set_camera(self.h, self._f(position), float(angle_x), float(angle_y))

    def finish(self):
        """Builds the BVH: 0, 1 (no triangles / bad call) or 2 (deeper than oracle_max_depth_limit(): never rendered)."""
        return oracle().oracle_scene_finish(self.h)

    def __del__(self):
        if getattr(self, "h", None) and _oracle is not None:
            _oracle.oracle_scene_destroy(self.h)

    def arrays(self):
        v = [_P(), _SZ(), _P(), _SZ(), _P(), _SZ(), _P(), _I(), _P(), _I(), _P(), _I()]
        oracle().oracle_scene_arrays(self.h, *[ctypes.byref(x) for x in v])
        grab = lambda p, n: np.frombuffer(ctypes.string_at(p.value, n), dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)
        return {"vertices": grab(v[0], v[1].value * 32), "faces": grab(v[2], v[3].value * 16),
                "nodes": grab(v[4], v[5].value * 32), "face_indices": grab(v[6], v[3].value * 4),
                "max_depth": v[7].value, "spheres": grab(v[8], v[9].value * 32), "materials": grab(v[10], v[11].value * 64)}

    def camera(self, w, h):
        out = (ctypes.c_float * 15)()
        oracle().oracle_camera(self.h, w, h, out)
        return np.array(out[:], dtype=np.float32)

    def render(self, w, h, spp, bounces, frame_index=0, seed=SEED, rng=None, last=None, rows=None, threads=0,
               stats=False):
        r0, r1 = rows if rows else (0, h)
        out = np.zeros((r1 - r0, w, 4), dtype=np.float32)
        st = np.zeros(8, dtype=np.uint64)
        rp = rng.ctypes.data if rng is not None else None
        lp = np.ascontiguousarray(last, dtype=np.float32).ctypes.data if last is not None else None
        keep = last
        code = oracle().oracle_render(self.h, w, h, spp, bounces, frame_index, seed, rp, lp, out.ctypes.data, r0, r1,
                                      threads, st.ctypes.data)
        del keep
        assert code == 0
        return (out, st) if stats else out

    def render_pending(self, w, h, spp, bounces, frame_index=0, seed=SEED, rng=None, last=None, threads=0):
        """render() of a whole frame plus, per pixel, the largest number of pending entries the DFS stack held over
        all of the pixel's rays (uint32 [h, w]); returns (frame, stats, pending), stats[7] the frame's maximum."""
        out = np.zeros((h, w, 4), dtype=np.float32)
        st = np.zeros(8, dtype=np.uint64)
        pend = np.zeros((h, w), dtype=np.uint32)
        rp = rng.ctypes.data if rng is not None else None
        keep = np.ascontiguousarray(last, dtype=np.float32) if last is not None else None
        code = oracle().oracle_render_pending(self.h, w, h, spp, bounces, frame_index, seed, rp,
                                              keep.ctypes.data if keep is not None else None, out.ctypes.data, 0, h, threads,
                                              st.ctypes.data, pend.ctypes.data)
        assert code == 0, "oracle_render_pending refused the scene or the frame"
        return out, st, pend


def oracle_rng_state(seed, sub):
    out = (ctypes.c_uint32 * 6)()
    oracle().oracle_rng_init(seed, sub, out)
    return np.array(out[:], dtype=np.uint32)


def oracle_rng_frame(seed, w, h, threads=0):
    out = np.zeros((h * w, 6), dtype=np.uint32)
    oracle().oracle_rng_init_frame(seed, w, h, out.ctypes.data, threads)
    return out


def product_scene(which="bunny", w=64, h=36):
    rt = load_rt()
    s = rt.Scene()
    s.setup(which)
    s.set_viewport(w, h)
    s.build()
    return s
