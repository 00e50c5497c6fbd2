"""Reference for the ray queries (rt_trace_rays): GetRayHit + BVHRayHit (main_raytracing.cu:33-109) restated
in Python over the reference arrays, in fp32 throughout.

The arithmetic is not re-invented here: the triangle and sphere tests and `normalize` are liboracle.so's
exported glm pieces (oracle_glm_tri_batch / oracle_glm_sphere_batch / oracle_glm_vec_batch, pinned bit for
bit against the reference's vendored glm by tests/test_oracle_glm.py); the slab test is IEEE float32
division with np.fmin / np.fmax (fminf / fmaxf semantics, Math.h:50-61); products and sums are single
numpy float32 operations (no contraction).  A leaf's triangles go through one batch call -- a test does not
depend on the closest distance, only the accept does -- so the 345-triangle and 12,318-triangle leaves
stay cheap; the accepts are then taken in leaf order.

trace(arrays, rays) returns complete 48-byte rt_hit records and this module's own counters, which
tests/test_query_cpu.py pins to the oracle's traversal statistics.
"""
import ctypes

import numpy as np

import rt_testlib as T

F32 = np.float32
_P, _I64 = ctypes.c_void_p, ctypes.c_int64
_bound = False


def _glm():
    global _bound
    L = T.oracle()
    if not _bound:
        L.oracle_glm_tri_batch.argtypes = [_I64, _P, _P, _P, _P, _P, _P, _P]
        L.oracle_glm_sphere_batch.argtypes = [_I64, _P, _P, _P, _P, _P, _P]
        L.oracle_glm_vec_batch.argtypes = [_I64, _P, _P, _P, _P]
        L.oracle_glm_tri_batch.restype = L.oracle_glm_sphere_batch.restype = L.oracle_glm_vec_batch.restype = None
        _bound = True
    return L


def _vec(a, b=None):
    """oracle_glm_vec_batch for one pair: (normalize(a), dot(a, b))."""
    a = np.ascontiguousarray(a, dtype=F32)
    b = np.ascontiguousarray(a if b is None else b, dtype=F32)
    s = np.zeros(1, dtype=F32)
    out = np.zeros(18, dtype=F32)
    _glm().oracle_glm_vec_batch(1, a.ctypes.data, b.ctypes.data, s.ctypes.data, out.ctypes.data)
    return out[0:3].copy(), out[6]


def normalize(v):
    return _vec(v)[0]


class Arrays:
    """The reference arrays as typed views.  `a`: a dict of byte buffers or typed arrays with nodes,
    face_indices, faces, vertices (OracleScene.arrays() / Scene.host_arrays()), spheres ((S, 8) words:
    position, radius, material as int32, padding) and materials ((M, 16) float32)."""

    def __init__(self, a):
        raw = lambda k, dt, cols: np.ascontiguousarray(a[k]).view(np.uint8).reshape(-1).view(dt).reshape(-1, cols)
        nodes = raw("nodes", np.uint32, 8)
        self.bmin = nodes[:, 0:3].view(F32).copy()
        self.bmax = nodes[:, 3:6].view(F32).copy()
        self.first = nodes[:, 6].astype(np.int64)
        self.count = nodes[:, 7].astype(np.int64)
        self.face_indices = raw("face_indices", np.uint32, 1)[:, 0].astype(np.int64)
        self.faces = raw("faces", np.uint32, 4)  # GPUFace: v0, v2, v1, material
        verts = raw("vertices", F32, 8)
        self.vpos = verts[:, 0:3].copy()
        self.vnrm = verts[:, 3:6].copy()
        sph = raw("spheres", np.uint32, 8) if len(a.get("spheres", ())) else np.zeros((0, 8), np.uint32)
        self.sph_c = np.ascontiguousarray(sph[:, 0:3].view(F32))
        self.sph_r = np.ascontiguousarray(sph[:, 3].view(F32))
        self.sph_mat = sph[:, 4].view(np.int32).copy()
        self._leaf = {}

    def leaf(self, node):
        """(face ids, v0, v1, v2 positions) of a leaf, gathered once."""
        got = self._leaf.get(node)
        if got is None:
            ids = self.face_indices[self.first[node]:self.first[node] + self.count[node]]
            f = self.faces[ids]
            got = (ids, np.ascontiguousarray(self.vpos[f[:, 0]]), np.ascontiguousarray(self.vpos[f[:, 2]]),
                   np.ascontiguousarray(self.vpos[f[:, 1]]))
            self._leaf[node] = got
        return got


COUNTERS = ("nodes", "tris", "tacc", "sacc", "hits", "misses")


def trace(arrays, rays):
    """rays: (N, 8) float32 rt_ray rows.  Returns (hits (N, 12) float32 rt_hit rows, counters dict, leaf size of
    each ray's final triangle hit (0 otherwise))."""
    A = arrays if isinstance(arrays, Arrays) else Arrays(arrays)
    L = _glm()
    rays = np.ascontiguousarray(rays, dtype=F32).reshape(-1, 8)
    n = rays.shape[0]
    hits = np.zeros((n, 12), dtype=F32)
    hits_u = hits.view(np.uint32)
    cnt = dict.fromkeys(COUNTERS, 0)
    leaf_size = np.zeros(n, dtype=np.int64)
    ns = A.sph_c.shape[0]
    s_hit, s_dist = np.zeros(max(ns, 1), np.int32), np.zeros(max(ns, 1), F32)
    with np.errstate(all="ignore"):
        for r in range(n):
            ro, tmax, rd = rays[r, 0:3].copy(), rays[r, 3], rays[r, 4:7].copy()
            best, kind, pid, bx, by, lsize = tmax, 0, 0, F32(0), F32(0), 0
            # the sphere loop, strict < (main_raytracing.cu:87-101)
            if ns:
                o_rep, d_rep = np.ascontiguousarray(np.broadcast_to(ro, (ns, 3))), np.ascontiguousarray(np.broadcast_to(rd, (ns, 3)))
                L.oracle_glm_sphere_batch(ns, o_rep.ctypes.data, d_rep.ctypes.data, A.sph_c.ctypes.data, A.sph_r.ctypes.data,
                                          s_hit.ctypes.data, s_dist.ctypes.data)
                for i in range(ns):
                    if s_hit[i]:
                        if s_dist[i] >= best:
                            continue
                        best, kind, pid = s_dist[i], 1, i
                        cnt["sacc"] += 1
            # BVHRayHit (main_raytracing.cu:33-81): right-first DFS, the slab test on the direction as given
            stack = [0]
            while stack:
                node = stack.pop()
                cnt["nodes"] += 1
                t1 = (A.bmin[node] - ro) / rd
                t2 = (A.bmax[node] - ro) / rd
                lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
                tmin = np.fmax(np.fmax(lo[0], lo[1]), lo[2])
                tmx = np.fmin(np.fmin(hi[0], hi[1]), hi[2])
                if not (tmx >= tmin and tmin < best and tmx > 0):
                    continue
                c = int(A.count[node])
                if c > 0:
                    ids, v0, v1, v2 = A.leaf(node)
                    o_rep = np.ascontiguousarray(np.broadcast_to(ro, (c, 3)))
                    d_rep = np.ascontiguousarray(np.broadcast_to(rd, (c, 3)))  # the batch normalises d itself
                    t_hit, t_out = np.zeros(c, np.int32), np.zeros((c, 3), F32)
                    L.oracle_glm_tri_batch(c, o_rep.ctypes.data, d_rep.ctypes.data, v0.ctypes.data, v1.ctypes.data,
                                           v2.ctypes.data, t_hit.ctypes.data, t_out.ctypes.data)
                    cnt["tris"] += c
                    for i in np.nonzero(t_hit)[0]:
                        dist = t_out[i, 2]
                        if dist >= best or dist < 0:
                            continue
                        best, kind, pid, bx, by, lsize = dist, 2, int(ids[i]), t_out[i, 0], t_out[i, 1], c
                        cnt["tacc"] += 1
                else:
                    stack.append(int(A.first[node]))
                    stack.append(int(A.first[node]) + 1)
            # `result.distance < max_distance`: a NaN distance is a miss
            if kind != 0 and best < tmax:
                cnt["hits"] += 1
                nd = normalize(rd)
                pos = ro + nd * best
                if kind == 1:
                    nrm = (pos - A.sph_c[pid]) / A.sph_r[pid]
                    mat = int(A.sph_mat[pid])
                else:
                    f = A.faces[pid]
                    bz = (F32(1.0) - bx) - by
                    nrm = normalize((A.vnrm[f[0]] * bx + A.vnrm[f[2]] * by) + A.vnrm[f[1]] * bz)
                    if _vec(nd, nrm)[1] >= 0:
                        nrm = -nrm
                    mat = int(f[3])
                    leaf_size[r] = lsize
                hits[r, 0] = best
                hits_u[r, 1:4] = (kind, pid, mat & 0xFFFFFFFF)
                hits[r, 4:7], hits[r, 7] = nrm, bx
                hits[r, 8:11], hits[r, 11] = pos, by
            else:
                cnt["misses"] += 1
                hits[r, 0] = tmax
    return hits, cnt, leaf_size


def camera_rays(cam15, width, height, jitter=None):
    """The (H*W, 8) rays of a frame from a 15-float GPUCamera (origin, viewport size, aspect, horizontal,
    vertical, lower-left corner): through the pixel centres, or with `jitter` (H*W, 2) the renderer's
    sample rays ((x + u) / W, (y + v) / H; rt_fast_body.h).  Ray i is pixel (i % W, i // W); tmax 1e30f."""
    cam = np.asarray(cam15, dtype=F32)
    co, ch, cv, cl = cam[0:3], cam[6:9], cam[9:12], cam[12:15]
    i = np.arange(width * height)
    x, y = (i % width).astype(F32), (i // width).astype(F32)
    ju = np.full(i.size, 0.5, F32) if jitter is None else np.asarray(jitter, F32)[:, 0]
    jv = np.full(i.size, 0.5, F32) if jitter is None else np.asarray(jitter, F32)[:, 1]
    ux = ((x + ju) / F32(width)).astype(F32)
    uy = ((y + jv) / F32(height)).astype(F32)
    rd = ((cl[None, :] + ch[None, :] * ux[:, None]) + cv[None, :] * uy[:, None]) - co[None, :]
    rays = np.zeros((i.size, 8), dtype=F32)
    rays[:, 0:3] = co
    rays[:, 3] = F32(1e30)
    rays[:, 4:7] = rd
    return rays


def frame_jitter(seed, width, height):
    """(H*W, 2) first two draws (u, v) of every pixel's RNG state curand_init(seed, y*W + x, 0)."""
    L = T.oracle()
    out = np.zeros((width * height, 2), dtype=F32)
    st = (ctypes.c_uint32 * 6)()
    uv = (ctypes.c_float * 2)()
    for p in range(width * height):
        L.oracle_rng_init(seed, p, st)
        L.oracle_rng_draws(st, 2, uv)
        out[p] = uv[0], uv[1]
    return out
