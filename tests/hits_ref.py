"""Reference for rt_trace_hits: rt_abi.h's rule restated in Python on query_ref.Arrays -- GetRayHit / BVHRayHit
(main_raytracing.cu:33-109) with the closest distance replaced by a list of K.  The arithmetic is query_ref's: the
oracle's glm batches for the sphere and triangle tests and for normalize, IEEE float32 division with np.fmin / np.fmax
for the slab test.  The one quantity the batches do not return, the sign of the triangle test's det, is formed here in
numpy float32 in rt_math.h's operation order (cross: a.y * b.z - b.y * a.z ...; dot: (x + y) + z).

trace(arrays, rays, k, flags) returns (hits (N, k, 12) float32 rt_hit rows, counts (N,) int32: the list's length, or
under COUNT_ALL the total).  With pending=True a third array follows: per ray, the most entries the kernel's stack
holds at once (rt_fast.h inner_step: a left child goes onto it when its box is entered at all -- exit >= entry and
exit > 0, whatever the bound -- and the right child is continued), read off this DFS whenever it enters a node."""
import numpy as np

import query_ref as Q

F32 = np.float32
CULL_BACK, CULL_FRONT, COUNT_ALL = 1, 2, 4


class HitList:
    """The list and its offer(), sequentially: arrival order breaks ties."""

    def __init__(self, k, tmax, count_all):
        self.k, self.tmax, self.count_all = k, F32(tmax), count_all
        self.entries = []  # (t, kind, id, bx, by)
        self.total = 0

    def bound(self):
        return self.entries[self.k - 1][0] if (not self.count_all and len(self.entries) >= self.k) else self.tmax

    def offer(self, t, kind, pid, bx=F32(0), by=F32(0)):
        if np.isnan(t) or t < 0 or not (t < self.bound()):
            return
        self.total += 1
        at = len(self.entries)
        for j, e in enumerate(self.entries):
            if e[0] > t:
                at = j
                break
        self.entries.insert(at, (F32(t), kind, pid, bx, by))
        del self.entries[self.k:]


def det_sign(nd, v0, v1, v2):
    """det = dot(v1 - v0, cross(nd, v2 - v0)) of glm's test for a batch of triangles, float32 operation by operation."""
    e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
    px = (nd[1] * e2[:, 2]).astype(F32) - (e2[:, 1] * nd[2]).astype(F32)
    py = (nd[2] * e2[:, 0]).astype(F32) - (e2[:, 2] * nd[0]).astype(F32)
    pz = (nd[0] * e2[:, 1]).astype(F32) - (e2[:, 0] * nd[1]).astype(F32)
    return ((e1[:, 0] * px).astype(F32) + (e1[:, 1] * py).astype(F32)).astype(F32) + (e1[:, 2] * pz).astype(F32)


def trace(arrays, rays, k, flags=0, pending=False):
    A = arrays if isinstance(arrays, Q.Arrays) else Q.Arrays(arrays)
    L = Q._glm()
    rays = np.ascontiguousarray(rays, dtype=F32).reshape(-1, 8)
    n = rays.shape[0]
    cull, count_all = flags & 3, bool(flags & COUNT_ALL)
    assert cull != 3 and 1 <= k <= 16
    hits = np.zeros((n, k, 12), dtype=F32)
    hits_u = hits.view(np.uint32)
    counts = np.zeros(n, dtype=np.int32)
    held_max = np.zeros(n, dtype=np.int32)
    ns = A.sph_c.shape[0]
    s_hit, s_dist = np.zeros(max(ns, 1), np.int32), np.zeros(max(ns, 1), F32)
    with np.errstate(all="ignore"):
        for r in range(n):
            ro, tmax, rd = rays[r, 0:3].copy(), rays[r, 3], rays[r, 4:7].copy()
            nd = Q.normalize(rd)
            lst = HitList(k, tmax, count_all)
            if ns:
                o_rep, d_rep = np.ascontiguousarray(np.broadcast_to(ro, (ns, 3))), np.ascontiguousarray(np.broadcast_to(rd, (ns, 3)))
                L.oracle_glm_sphere_batch(ns, o_rep.ctypes.data, d_rep.ctypes.data, A.sph_c.ctypes.data, A.sph_r.ctypes.data,
                                          s_hit.ctypes.data, s_dist.ctypes.data)
                for i in range(ns):
                    if s_hit[i]:
                        lst.offer(s_dist[i], 1, i)
            def slab(node):
                t1 = (A.bmin[node] - ro) / rd
                t2 = (A.bmax[node] - ro) / rd
                lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
                return np.fmax(np.fmax(lo[0], lo[1]), lo[2]), np.fmin(np.fmin(hi[0], hi[1]), hi[2])

            stack, held = [0], [False]  # held: whether the kernel's stack would hold that entry (pending only)
            while stack:
                node = stack.pop()
                tmin, tmx = slab(node)
                if pending:
                    held.pop()
                if not (tmx >= tmin and tmin < lst.bound() and tmx > 0):
                    continue
                if pending:
                    held_max[r] = max(held_max[r], sum(held))
                c = int(A.count[node])
                if c > 0:
                    ids, v0, v1, v2 = A.leaf(node)
                    o_rep = np.ascontiguousarray(np.broadcast_to(ro, (c, 3)))
                    d_rep = np.ascontiguousarray(np.broadcast_to(rd, (c, 3)))  # the batch normalises d itself
                    t_hit, t_out = np.zeros(c, np.int32), np.zeros((c, 3), F32)
                    L.oracle_glm_tri_batch(c, o_rep.ctypes.data, d_rep.ctypes.data, v0.ctypes.data, v1.ctypes.data,
                                           v2.ctypes.data, t_hit.ctypes.data, t_out.ctypes.data)
                    idx = np.nonzero(t_hit)[0]
                    if cull and idx.size:
                        det = det_sign(nd, v0[idx], v1[idx], v2[idx])
                        assert (np.abs(det) > F32(1.1920928955078125e-07)).all()  # the test accepted them
                        idx = idx[(det > 0) if cull == CULL_BACK else (det < 0)]
                    for i in idx:
                        lst.offer(t_out[i, 2], 2, int(ids[i]), t_out[i, 0], t_out[i, 1])
                else:
                    stack.append(int(A.first[node]))
                    stack.append(int(A.first[node]) + 1)
                    if pending:
                        lmin, lmx = slab(int(A.first[node]))
                        held += [bool(lmx >= lmin and lmx > 0), False]
            hits[r, :, 0] = tmax
            for j, (t, kind, pid, bx, by) in enumerate(lst.entries):
                pos = ro + nd * t
                if kind == 1:
                    nrm = (pos - A.sph_c[pid]) / A.sph_r[pid]
                    mat = int(A.sph_mat[pid])
                else:
                    f = A.faces[pid]
                    bz = (F32(1.0) - bx) - by
                    nrm = Q.normalize((A.vnrm[f[0]] * bx + A.vnrm[f[2]] * by) + A.vnrm[f[1]] * bz)
                    if Q._vec(nd, nrm)[1] >= 0:
                        nrm = -nrm
                    mat = int(f[3])
                hits[r, j, 0] = t
                hits_u[r, j, 1:4] = (kind, pid, mat & 0xFFFFFFFF)
                hits[r, j, 4:7], hits[r, j, 7] = nrm, bx
                hits[r, j, 8:11], hits[r, j, 11] = pos, by
            counts[r] = lst.total if count_all else len(lst.entries)
    return (hits, counts, held_max) if pending else (hits, counts)
