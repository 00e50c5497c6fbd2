"""The scene: the Scene class (host geometry, camera, upload), the BVH and mirror builders' entry points, their
build options, and the hooks for foreign GPUScenes."""
import ctypes

import numpy as np
import torch

from . import _abi
from ._abi import ASSETS_DIR, SCENES, BuildOptions, GPUCamera, GPUMaterial, RTError, _check, lib
from ._args import _f3, _stream_ptr


def _sized_copy(handle, name, shape_of, dtype=np.float32):
    """The array of a query-the-size-then-copy getter rt_scene_<name>(handle, out, &n): shape_of(n) of `dtype`."""
    fn, n = getattr(lib(), "rt_scene_" + name), ctypes.c_size_t()
    _check(fn(handle, None, ctypes.byref(n)), "rt_scene_" + name)
    out = np.zeros(shape_of(n.value), dtype=dtype)
    if n.value:
        _check(fn(handle, out.ctypes.data, ctypes.byref(n)), "rt_scene_" + name)
    return out


class Scene:
    """RayTracing::Scene mirror (RayTracing/Scene.h:87-129)."""

    def __init__(self):
        self.handle = lib().rt_scene_create()
        if not self.handle:
            raise RTError("rt_scene_create failed")

    def __del__(self):
        loaded = getattr(_abi, "_lib", None)  # at interpreter shutdown the module and the library may be gone already
        if getattr(self, "handle", None) and loaded is not None:
            loaded.rt_scene_destroy(self.handle)
            self.handle = None

    # --- building (Scene.cpp:46-139) -------------------------------------------------
    def add_material(self, albedo=(0, 0, 0), emissive=(0, 0, 0), specular=(0, 0, 0, 0), roughness=0.9,
                     specular_percent=0.0, ior=1.0):
        m = GPUMaterial()
        m.albedo[:] = [*map(float, albedo[:3]), 1.0]
        m.emissive[:] = [*map(float, emissive[:3]), 1.0]
        m.specular[:] = [*map(float, (list(specular) + [0.0])[:4])]
        m.roughness, m.specular_percent, m.IOR = roughness, specular_percent, ior
        return lib().rt_scene_add_material(self.handle, ctypes.byref(m))

    def add_triangle(self, a, b, c, material=0):
        lib().rt_scene_add_triangle(self.handle, _f3(a), _f3(b), _f3(c), material)

    def add_quad(self, a, b, c, d, material=0):
        lib().rt_scene_add_quad(self.handle, _f3(a), _f3(b), _f3(c), _f3(d), material)

    def add_sphere(self, position, radius, material=0):
        lib().rt_scene_add_sphere(self.handle, _f3(position), float(radius), material)

    def add_loaded_scene(self, mesh_path, transform, material=0):
        t = (ctypes.c_float * 16)(*[float(x) for x in transform])
        _check(lib().rt_scene_add_mesh_file(self.handle, mesh_path.encode(), t, material), "add_loaded_scene")

    def set_environment(self, path):
        _check(lib().rt_scene_set_environment_file(self.handle, path.encode()), "set_environment")

    def environment(self):
        """Host copy of the level-0 cube texels [6, size, size, 4] (None when no sky is set)."""
        texels, n = ctypes.c_void_p(), ctypes.c_int()
        _check(lib().rt_scene_environment(self.handle, ctypes.byref(texels), ctypes.byref(n)), "rt_scene_environment")
        if not texels.value:
            return None
        k = n.value
        buf = ctypes.string_at(texels.value, 6 * k * k * 16)
        return np.frombuffer(buf, dtype=np.float32).reshape(6, k, k, 4).copy()

    def setup(self, which="bunny", assets_dir=ASSETS_DIR):
        """CUDARayTracer::SetupCornellBox + SetupStanfordBunny (or the config-4/5 scenes)."""
        _check(lib().rt_scene_setup(self.handle, SCENES[which], assets_dir.encode()), f"setup({which})")

    def setup_plane(self, n=708, assets_dir=ASSETS_DIR):
        _check(lib().rt_scene_setup_plane(self.handle, int(n), assets_dir.encode()), f"setup_plane({n})")

    def set_camera(self, position=(0, 0, 0), angle_x=0.0, angle_y=180.0):
        lib().rt_scene_set_camera(self.handle, _f3(position), float(angle_x), float(angle_y))

    def set_viewport(self, width, height):
        lib().rt_scene_set_viewport(self.handle, int(width), int(height))

    def upload(self, rng_state_ptr):
        """Scene::Upload (Scene.cpp:182-234): BVH build if dirty, H2D copies, GPUScene fill."""
        _check(lib().rt_scene_upload(self.handle, ctypes.c_void_p(rng_state_ptr)), "upload")

    @property
    def gpu(self):
        return lib().rt_scene_gpu(self.handle)

    def build(self):
        """Host half of upload (camera + BVH) with no device work."""
        lib().rt_scene_build(self.handle)

    def camera(self):
        c = GPUCamera()
        lib().rt_scene_camera(self.handle, ctypes.byref(c))
        return c

    def max_depth(self):
        return lib().rt_scene_bvh_max_depth(self.handle)

    def mirror(self, trees=False):
        """The kernel's triangle mirror built on the host (mirror.h): leaf-ordered (N,12) float32
        records (v0, e1, e2, face id bits, pair/tree index, flag); with trees=True also the leaf
        trees: nodes (K,16) and their triangle records (M,12) (leaftree.h)."""
        n = [ctypes.c_size_t() for _ in range(3)]
        _check(lib().rt_scene_mirror_info(self.handle, *[ctypes.byref(x) for x in n]), "rt_scene_mirror_info")
        tris, tree, ltris = (np.zeros((x.value, k), dtype=np.float32) for x, k in zip(n, (12, 16, 12)))
        _check(lib().rt_scene_mirror_copy(self.handle, tris.ctypes.data, tree.ctypes.data, ltris.ctypes.data),
               "rt_scene_mirror_copy")
        return (tris, tree, ltris) if trees else tris

    def mirror_nodes(self):
        """The traversal's private node array (mirror.h nodes) as (N, 8) float32 (uint32 view for
        first / count)."""
        return _sized_copy(self.handle, "mirror_nodes", lambda n: (n, 8))

    def mirror_face_leaf(self):
        """Scenes with big leaves: each face's leaf in the private node array (uint32; 0xffffffff none,
        0xfffffffe two leaves), the deferred leaves' guard table (rt_fast.h); empty otherwise."""
        return _sized_copy(self.handle, "mirror_face_leaf", lambda n: n, np.uint32)

    def mirror_twins(self):
        """The big leaves' twin records (mirror.h): quads (Q, 28) and units (U, 16) float32."""
        nq, nu = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().rt_scene_mirror_twins(self.handle, None, ctypes.byref(nq), None, ctypes.byref(nu)), "rt_scene_mirror_twins")
        q = np.zeros((nq.value, 28), dtype=np.float32)
        u = np.zeros((nu.value, 16), dtype=np.float32)
        _check(lib().rt_scene_mirror_twins(self.handle, q.ctypes.data, ctypes.byref(nq), u.ctypes.data, ctypes.byref(nu)),
               "rt_scene_mirror_twins")
        return q, u

    def mirror_leaf_twin(self, first):
        """The twin record (mirror.h pairs) of the big leaf whose first leaf-ordered record is `first`: 12 float32
        (KD, KE, KDD, KDD1, lo.xyz, 0, hi.xyz, 0)."""
        rec = np.zeros(12, dtype=np.float32)
        _check(lib().rt_scene_mirror_leaf_twin(self.handle, int(first), rec.ctypes.data), "rt_scene_mirror_leaf_twin")
        return rec

    def materials(self):
        """Host copy of the GPUMaterial array as (M, 16) float32: albedo 0-3, emissive 4-7, specular 8-11,
        roughness, specular_percent, IOR, padding (what rt_hit.material indexes)."""
        return _sized_copy(self.handle, "materials", lambda n: (n, 16))

    def spheres(self):
        """Host copy of the sphere array as (S, 8) float32: centre 0-2, radius, material (an int32), padding."""
        return _sized_copy(self.handle, "spheres", lambda n: (n, 8))

    def host_arrays(self):
        """numpy copies of the host arrays: nodes (N,8) f32/u32 view, face indices, vertices, faces."""
        ptrs = [ctypes.c_void_p() for _ in range(4)]
        counts = [ctypes.c_size_t() for _ in range(3)]
        lib().rt_scene_host_arrays(self.handle, ctypes.byref(ptrs[0]), ctypes.byref(counts[0]), ctypes.byref(ptrs[1]),
                                   ctypes.byref(counts[1]), ctypes.byref(ptrs[2]), ctypes.byref(counts[2]),
                                   ctypes.byref(ptrs[3]))

        def grab(p, nbytes):
            if not p.value or nbytes == 0:
                return np.zeros(0, dtype=np.uint8)
            return np.frombuffer(ctypes.string_at(p.value, nbytes), dtype=np.uint8).copy()

        nn, nf, nv = counts[0].value, counts[1].value, counts[2].value
        return {"nodes": grab(ptrs[0], nn * 32), "face_indices": grab(ptrs[1], nf * 4),
                "vertices": grab(ptrs[2], nv * 32), "faces": grab(ptrs[3], nf * 16)}


def mirror_build_check(nodes, face_indices, faces, vertices):
    """rt_mirror_build_check: the host mirror of raw reference arrays (numpy: nodes (N,8) 32-bit, face
    indices u32, faces (F,4) u32, vertices (V,8) f32) -> (words 10-11 of every record as (n, 2) uint32,
    whether twin records were built)."""
    nodes, fi = np.ascontiguousarray(nodes), np.ascontiguousarray(face_indices, dtype=np.uint32)
    faces, vertices = np.ascontiguousarray(faces), np.ascontiguousarray(vertices)
    meta = np.zeros((fi.size, 2), dtype=np.uint32)
    tw = ctypes.c_int(0)
    _check(lib().rt_mirror_build_check(nodes.ctypes.data, nodes.shape[0], fi.ctypes.data, fi.size, faces.ctypes.data,
                                       faces.shape[0], vertices.ctypes.data, vertices.shape[0], meta.ctypes.data,
                                       ctypes.byref(tw)), "rt_mirror_build_check")
    return meta, bool(tw.value)


def entry_table_builds():
    """Entry tables rt_render has built so far in this process (rt_entry_table_builds)."""
    return int(lib().rt_entry_table_builds())


def bvh_build_device(vertices, faces, stream=None):
    """BVH::Calculate on the GPU (rt_bvh_build_device) from device tensors of GPUVertex (N,8) f32
    and GPUFace (F,4) u32 rows; returns (nodes (2F-1, 8) f32 device tensor, face_indices (F,) int32
    device tensor, node_count, max_depth)."""
    nf = faces.shape[0]
    nodes = torch.empty((max(1, 2 * nf - 1), 8), dtype=torch.float32, device=faces.device)
    fi = torch.empty((nf,), dtype=torch.int32, device=faces.device)
    count, depth = ctypes.c_uint32(0), ctypes.c_int(0)
    _check(lib().rt_bvh_build_device(vertices.data_ptr(), vertices.shape[0], faces.data_ptr(), nf, nodes.data_ptr(),
                                     fi.data_ptr(), ctypes.byref(count), ctypes.byref(depth), _stream_ptr(stream)),
           "rt_bvh_build_device")
    return nodes, fi, count.value, depth.value


def build_options():
    """Current rt_build_options (a BuildOptions)."""
    o = BuildOptions()
    lib().rt_get_build_options(ctypes.byref(o))
    return o


def set_build_options(**changes):
    """rt_set_build_options with the given fields changed (no arguments: the defaults)."""
    if not changes:
        _check(lib().rt_set_build_options(None), "rt_set_build_options")
        return
    o = build_options()
    for k, v in changes.items():
        setattr(o, k, v)
    _check(lib().rt_set_build_options(ctypes.byref(o)), "rt_set_build_options")


def foreign_mirror_wait(gpu_scene):
    """rt_foreign_mirror_wait: block until the background mirror build of a foreign GPUScene (a
    ctypes GPUScene filled by the caller) has finished; the next render installs it."""
    _check(lib().rt_foreign_mirror_wait(ctypes.byref(gpu_scene)), "rt_foreign_mirror_wait")


def foreign_last_tracer(gpu_scene):
    """rt_foreign_last_tracer: 1 production tracer, 0 reference layout (fingerprint mismatch),
    -1 no mirror yet (test diagnostics; synchronises the device)."""
    return int(lib().rt_foreign_last_tracer(ctypes.byref(gpu_scene)))


def cluster_cull_host(origin, nd, best, node):
    """The render kernel's leaf-tree cull predicate (rt_fast.h cluster_cull) on the host."""
    o = np.ascontiguousarray(origin, dtype=np.float32)
    d = np.ascontiguousarray(nd, dtype=np.float32)
    k = np.ascontiguousarray(node, dtype=np.float32)
    return bool(lib().rt_cluster_cull_host(o.ctypes.data, d.ctypes.data, float(best), k.ctypes.data))
