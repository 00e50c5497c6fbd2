"""The twin test with its bounds hoisted out of the big-leaf loops (rt_fast.h twin_rejected_pre, twin_visit; the
leaf's twin record of mirror.h), settled on the CPU through the host hooks, which run the kernels' own source:

 * the hoisted form on bounds (KD, KE, DN) at 1x, 4x and 64x a triangle's own never declares rejected a twin that
   glm's predicate accepts, over the rays of tests/test_scene.py (edges, vertices, grazing, random) and of
   tests/test_adversarial_cpu.py (slivers, mixed scales, |o - v0|_1 from 0 to 2^12), and the packed evaluation of
   the shared-leaf loop agrees with the scalar one on every one of them;
 * the per-unit wrapper twin_rejected answers exactly as the function it replaces (restated here in numpy fp32);
 * a leaf's record bounds every one of its units: KD >= kd, KE >= ke, KDD >= kd + 2^-90, KDD1 >= kdd (1 + 2^-20),
   the box holds every v0, and twin_visit's DN >= every unit's computed |o - v0|_1 -- for the bunny's and the
   4-bunny's big leaves and for the pinwheel leaf, whose largest twin's kd is more than 2^20 times its smallest.
"""
import ctypes

import numpy as np
import pytest

import adversarial_cases as AC
import rt_testlib as T

F32 = np.float32
SCALES = (1.0, 4.0, 64.0)


@pytest.fixture(scope="module")
def rt():
    return T.load_rt()


@pytest.fixture(scope="module")
def scene_a(rt):
    case = AC.build_case(rt, "A")
    return case, AC.ray_set(case, case.arrays())


def _normalized(rays):
    d = rays[:, 4:7].astype(np.float64)
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)


def scene_rays(rec, gen, trials=60):
    """tests/test_scene.py test_twin_quads_and_bound's rays for one triangle record: (origins, directions)."""
    r = np.ascontiguousarray(rec, dtype=F32)
    v0, e1, e2 = r[:3], r[3:6], r[6:9]
    pts = [v0, v0 + e1, v0 + e2, v0 + 0.5 * e1, v0 + 0.5 * e2, v0 + 0.5 * (e1 + e2)]
    nrm = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    nrm /= np.linalg.norm(nrm) + 1e-300
    os_, ds = [], []
    for trial in range(trials):
        target = pts[trial % len(pts)] + gen.normal(size=3) * 10.0 ** gen.uniform(-7, -1) * np.abs(e1).max()
        o = (target + gen.normal(size=3) * 10.0 ** gen.uniform(-1, 2)).astype(F32)
        d = (target - o).astype(np.float64)
        if trial % 3 == 1:
            d -= nrm * (d @ nrm) * (1 - 10.0 ** gen.uniform(-7, -1))
        if trial % 5 == 4:
            d = gen.normal(size=3)
        os_.append(o)
        ds.append((d / np.linalg.norm(d)).astype(F32))
    return np.ascontiguousarray(os_, F32), np.ascontiguousarray(ds, F32)


def unit_bounds(units):
    return {units[k, :9].tobytes(): (units[k, 12], units[k, 13]) for k in range(len(units)) if units[k, 12] >= 0}


def twin_rejected_before(det, u, v, uv, dn, kd, ke):
    """The function the wrapper replaces, operation for operation in fp32."""
    one_up, one_down = F32(1.0) + F32(2.0 ** -20), F32(1.0) - F32(2.0 ** -20)
    tiny, eps = F32(2.0 ** -90), F32(1.1920928955078125e-07)
    neg = np.signbit(det)
    ad = np.abs(det)
    su, sv, suv = (-u if neg else u), (-v if neg else v), (-uv if neg else uv)
    with np.errstate(all="ignore"):
        if not (((ad + np.abs(su)) + np.abs(sv)) + dn < F32(2.0 ** 100)):
            return False
        m = ke * dn + tiny
        kdd = kd + tiny
        top = (ad + kdd) * one_up
        if top <= eps:
            return True
        if not (ad > kdd * one_up):
            return False
        if sv < -m or su < -m:
            return True
        if sv > ((ad + kdd) + m) * one_up:
            return True
        return bool(suv * one_down > ((ad + kdd) + F32(2.001) * m) * one_up)


def glm_values(rec, o, nd):
    """(det, u, v, u + v, |o - v0|_1) of glm's test in test_triangle's fp32 operation order."""
    v0, e1, e2 = rec[:3], rec[3:6], rec[6:9]

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    with np.errstate(all="ignore"):
        p = cross(nd, e2)
        det = dot(e1, p)
        dist = o - v0
        u = dot(dist, p)
        v = dot(nd, cross(dist, e1))
        return det, u, v, u + v, (np.abs(dist[0]) + np.abs(dist[1])) + np.abs(dist[2])


def sweep(lib, recs, bounds_of, rays_of):
    """Every (record, ray) through the plain hook and the hoisted one at each scale; returns the counts."""
    plain, hoisted = lib.rt_twin_check_host, lib.rt_twin_check_bounds_host
    total = bad = packed_differs = wrapper_differs = 0
    decided = dict.fromkeys(SCALES, 0)
    b = np.zeros(3, F32)
    for rec in recs:
        rec = np.ascontiguousarray(rec, F32)
        kd, ke = bounds_of(rec)
        o, nd = rays_of(rec)
        for r in range(len(o)):
            det, u, v, uv, dn = glm_values(rec, o[r], nd[r])
            was = plain(rec.ctypes.data, o[r].ctypes.data, nd[r].ctypes.data)
            wrapper_differs += bool(was & 1) != twin_rejected_before(det, u, v, uv, dn, kd, ke)
            total += 1
            for s in SCALES:
                b[:] = (kd * F32(s), ke * F32(s), dn * F32(s))
                got = hoisted(rec.ctypes.data, o[r].ctypes.data, nd[r].ctypes.data, b.ctypes.data)
                assert (got & 6) == (was & 6)
                bad += (got & 3) == 3
                packed_differs += (got >> 3) & 1
                decided[s] += got & 1
                if s == 1.0:
                    wrapper_differs += (got & 1) != (was & 1)  # the same bounds through either entry
                else:
                    assert not (got & 1) or (was & 1), "a weaker bound decided a twin the triangle's own did not"
    return total, bad, packed_differs, wrapper_differs, decided


@pytest.mark.parametrize("which", ["bunny", "bunny4"])
def test_hoisted_form_on_scene_rays(rt, which):
    s = rt.Scene()
    s.setup(which)
    s.build()
    tris = s.mirror()
    tu = tris.view(np.uint32).reshape(-1, 12)
    _, units = s.mirror_twins()
    own = unit_bounds(units)
    nodes = s.host_arrays()["nodes"].view(np.uint32).reshape(-1, 8)
    counts = {int(n[6]): int(n[7]) for n in nodes if n[7] > 0}
    leads = [i for i in range(tu.shape[0]) if tu[i, 11] in (1, 3)]
    f = max(leads, key=lambda x: counts[x])
    recs = [r for r in tris[f:f + counts[f]] if r[:9].tobytes() in own][:60]
    gen = np.random.default_rng(7)
    total, bad, packed, wrapper, decided = sweep(rt.lib(), recs, lambda r: own[r[:9].tobytes()], lambda r: scene_rays(r, gen))
    print(f"{which}: {total} (triangle, ray) pairs, decided at 1x/4x/64x: {[decided[s] for s in SCALES]}")
    assert bad == 0, f"{bad} twins declared rejected by the hoisted form but accepted by glm's predicate"
    assert packed == 0, f"{packed} packed evaluations differ from the scalar one"
    assert wrapper == 0, f"{wrapper} answers of the per-unit wrapper differ from the function it replaces"
    assert decided[1.0] > 0.5 * total and decided[64.0] > 0.25 * total, decided


def test_hoisted_form_on_the_pinwheel(rt, scene_a):
    """Slivers, mixed scales and |o - v0|_1 from 0 to 2^12 (families 1-3 of the adversarial rays)."""
    case, rs = scene_a
    _, first, count = case.big_leaf()
    recs = np.ascontiguousarray(case.scene.mirror()[first:first + count])
    _, units = case.scene.mirror_twins()
    own = unit_bounds(units)
    pick = np.flatnonzero(rs.family <= 3)[::3]
    o, nd = np.ascontiguousarray(rs.rays[pick, 0:3]), _normalized(rs.rays[pick])
    assert np.isfinite(nd).all()
    with_twin = [r for r in recs if r[:9].tobytes() in own]
    assert len(with_twin) == count // 2
    total, bad, packed, wrapper, decided = sweep(rt.lib(), with_twin, lambda r: own[r[:9].tobytes()], lambda r: (o, nd))
    print(f"pinwheel: {total} pairs, decided at 1x/4x/64x: {[decided[s] for s in SCALES]}")
    assert total >= 10000
    assert bad == 0, f"{bad} twins declared rejected by the hoisted form but accepted by glm's predicate"
    assert packed == 0 and wrapper == 0, (packed, wrapper)
    assert 0 < decided[64.0] <= decided[4.0] <= decided[1.0] < total


def leaf_record_holds(rt, scene, first, count, origins):
    tris = scene.mirror()
    tu = tris.view(np.uint32).reshape(-1, 12)
    _, units = scene.mirror_twins()
    ub, nu = int(tu[first + 2, 10]), int(tu[first + 2, 11])
    un = units[ub:ub + nu]
    rec = scene.mirror_leaf_twin(first)
    KD, KE, KDD, KDD1, lo, hi = rec[0], rec[1], rec[2], rec[3], rec[4:7], rec[8:11]
    twins = un[un[:, 12] >= 0]
    assert len(twins) > 0
    tiny, one_up = F32(2.0 ** -90), F32(1.0) + F32(2.0 ** -20)
    assert KD == twins[:, 12].max() and KE == twins[:, 13].max()
    kdd = twins[:, 12] + tiny
    assert (KDD >= kdd).all() and (KDD1 >= kdd * one_up).all() and np.float64(KDD1) >= np.float64(KDD) * (1 + 2.0 ** -20)
    assert (lo <= un[:, 0:3]).all() and (un[:, 0:3] <= hi).all()
    assert np.array_equal(lo, un[:, 0:3].min(axis=0)) and np.array_equal(hi, un[:, 0:3].max(axis=0))
    visit = rt.lib().rt_twin_visit_host
    out = np.zeros(3, F32)
    for o in origins:
        o = np.ascontiguousarray(o, F32)
        visit(o.ctypes.data, lo.ctypes.data, hi.ctypes.data, ctypes.c_float(float(KE)), out.ctypes.data)
        with np.errstate(all="ignore"):
            d = np.abs(o[None, :] - un[:, 0:3])
            dn = (d[:, 0] + d[:, 1]) + d[:, 2]
            assert (out[0] >= dn).all(), (o, out[0], dn.max())
            m = twins[:, 13] * dn[un[:, 12] >= 0] + tiny
            assert (out[1] >= m).all() and (out[2] >= F32(2.001) * m).all()
            assert out[1] == KE * out[0] + tiny and out[2] == F32(2.001) * out[1]
    return twins[:, 12].max() / twins[twins[:, 12] > 0, 12].min()  # (a degenerate triangle's kd is 0)


def origins_around(lo, hi, gen, n=200):
    """Origins inside, on and far outside the box, up to 2^12 away, and at its corners and centre."""
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) + 1e-6
    pts = [c, lo, hi, np.array([lo[0], hi[1], lo[2]])]
    for _ in range(n):
        pts.append(c + gen.uniform(-1, 1, size=3) * h * 2.0 ** gen.uniform(-4, 12, size=3))
        pts.append(c + gen.normal(size=3) * 2.0 ** gen.uniform(-10, 12))
    return np.asarray(pts, F32)


@pytest.mark.parametrize("which", ["bunny", "bunny4"])
def test_leaf_records_of_the_bunnies(rt, which):
    s = rt.Scene()
    s.setup(which)
    s.build()
    tu = s.mirror().view(np.uint32).reshape(-1, 12)
    nodes = s.host_arrays()["nodes"].view(np.uint32).reshape(-1, 8)
    counts = {int(n[6]): int(n[7]) for n in nodes if n[7] > 0}
    leads = [i for i in range(tu.shape[0]) if tu[i, 11] in (1, 3)]
    assert leads
    gen = np.random.default_rng(11)
    for f in leads:
        rec = s.mirror_leaf_twin(f)
        spread = leaf_record_holds(rt, s, f, counts[f], origins_around(rec[4:7], rec[8:11], gen))
        print(f"{which}: leaf of {counts[f]} triangles, kd max / min {spread:.1f}")


def test_leaf_record_with_an_oversized_twin(rt, scene_a):
    """The pinwheel leaf mixes edges from 2^-8 to 2^5: its largest kd dwarfs its smallest, the case in which the
    leaf-wide bound is weakest -- and still a bound."""
    case, rs = scene_a
    _, first, count = case.big_leaf()
    rec = case.scene.mirror_leaf_twin(first)
    origins = np.concatenate([origins_around(rec[4:7], rec[8:11], np.random.default_rng(13)), rs.rays[::97, 0:3]])
    spread = leaf_record_holds(rt, case.scene, first, count, origins)
    print(f"pinwheel: kd max / min {spread:.3g}")
    assert spread > 2.0 ** 20
