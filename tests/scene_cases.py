"""Caller-built scenes, as plain data, for the oracle-checked frames of tests/test_user_scenes_cpu.py and
tests/test_gpu_user_scenes.py.

A case is a dict: `materials` (dicts of the six GPUMaterial fields), `prims` (("quad", a, b, c, d, material),
("tri", a, b, c, material), ("sphere", centre, radius, material)), `camera` (position, angle_x, angle_y), `sky`
(True: assets/sunset_cube128.bin, False: none), `width` / `height` / `spp` / `bounces`, and `expect`: what the
case is for, asserted on the oracle alone by the CPU tests before anything is launched --

    lean          the default frame runs the lean kernel (the mirror has big-leaf records); False: MODE 17 general
    depth         the BVH's depth, exactly
    fast          the mirror's filtered-range flag (absent: 1)
    seen          materials that must be the first hit of >= 16 pixel-centre rays (absent: every material)
    hits          exact number of pixel-centre rays that hit anything (the all-sky pose: 0)
    inside        a sphere index: >= 16 pixel-centre rays' first hit is that sphere
    refused       the depth makes every entry point (and the oracle's builder) refuse the scene: never rendered

apply_product / apply_oracle put one description into rt.Scene and into the oracle's builder: the only two
places that read a case, so neither side can be built from something the other did not get.

Viewports: neither side a multiple of the 16-pixel render tile, the pixel count no multiple of 64.
"""
import os

import rt_testlib as T

SKY = os.path.join(T.ASSETS, "sunset_cube128.bin")
SPP, BOUNCES, FRAMES = 2, 6, 2  # frame 0 plus one progressive frame


def mat(albedo=(0.0, 0.0, 0.0), emissive=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0, 0.0), roughness=0.9,
        specular_percent=0.0, ior=1.0):
    return {"albedo": tuple(albedo), "emissive": tuple(emissive), "specular": tuple(specular), "roughness": roughness,
            "specular_percent": specular_percent, "ior": ior}


def material_floats(m):
    """The 16 floats of the GPUMaterial rt.Scene.add_material builds from the same fields (alpha 1 on albedo and
    emissive, the specular colour's fourth component as given, padding 0)."""
    return [*m["albedo"][:3], 1.0, *m["emissive"][:3], 1.0, *(list(m["specular"]) + [0.0])[:4], m["roughness"],
            m["specular_percent"], m["ior"], 0.0]


def _apply(case, add_material, add):
    for m in case["materials"]:
        add_material(m)
    for p in case["prims"]:
        add[p[0]](*p[1:])


def apply_product(rt, case):
    """The case as an rt.Scene (viewport and camera set, nothing built or uploaded yet)."""
    s = rt.Scene()
    _apply(case, lambda m: s.add_material(m["albedo"], m["emissive"], m["specular"], m["roughness"], m["specular_percent"],
                                          m["ior"]),
           {"quad": s.add_quad, "tri": s.add_triangle, "sphere": s.add_sphere})
    if case["sky"]:
        s.set_environment(SKY)
    s.set_camera(*case["camera"])
    s.set_viewport(case["width"], case["height"])
    return s


def apply_oracle(case):
    """(T.OracleScene, finish code): the case through the oracle's builder; code 2 = refused for its depth."""
    o = T.OracleScene(None)
    _apply(case, lambda m: o.add_material(material_floats(m)),
           {"quad": o.add_quad, "tri": o.add_triangle, "sphere": o.add_sphere})
    o.set_sky(SKY if case["sky"] else None)
    o.set_camera(*case["camera"])
    return o, o.finish()


def case(name, materials, prims, camera, sky, size=(37, 19), **expect):
    return {"name": name, "materials": materials, "prims": prims, "camera": camera, "sky": sky, "width": size[0],
            "height": size[1], "spp": SPP, "bounces": BOUNCES, "expect": expect}


# ------------------------------------------------------------------------------------------------------
# the material room
# ------------------------------------------------------------------------------------------------------
WHITE, RED, LIGHT = 0, 1, 2
ROOM_LO, ROOM_HI = (-8.0, -6.0, -4.0), (8.0, 6.0, 20.0)
GRID_SP, GRID_ROUGH = (0.0, 0.5, 1.0), (0.0, 0.2, 1.0)


def room_materials():
    m = [mat(albedo=(0.7, 0.7, 0.7)), mat(albedo=(0.7, 0.2, 0.2)), mat(emissive=(6.0, 6.0, 6.0))]
    for sp in GRID_SP:  # 3 .. 11: specular_percent x roughness
        for rough in GRID_ROUGH:
            m.append(mat(albedo=(0.8, 0.6, 0.3), specular=(0.9, 0.9, 0.9, 0.0), specular_percent=sp, roughness=rough))
    m.append(mat(albedo=(1.5, 1.5, 1.5)))  # 12: survival probability above 1
    m.append(mat(albedo=(0.0, 0.0, 0.0), emissive=(2.0, 1.0, 0.5)))  # 13: p = 0, the path always stops
    m.append(mat(albedo=(0.5, 0.5, 0.9), specular=(0.0, 0.0, 0.0, 0.0), specular_percent=1.0, roughness=0.3))  # 14
    return m


def room_sphere(i):
    """Sphere i of the 4 x 3 grid in front of the default camera: (centre, radius)."""
    return (-4.05 + 2.7 * (i % 4), -2.7 + 2.7 * (i // 4), 5.0), 1.2


def room_prims(right_wall):
    lo, hi = ROOM_LO, ROOM_HI
    q = []

    def wall(axis, at, material, times=1):
        u, v = [k for k in range(3) if k != axis]
        corners = []
        for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
            p = [0.0, 0.0, 0.0]
            p[axis], p[u], p[v] = at, (hi[u] if a else lo[u]), (hi[v] if b else lo[v])
            corners.append(tuple(p))
        q.extend([("quad", *corners, material)] * times)

    wall(0, lo[0], RED)
    if right_wall:
        wall(0, hi[0], WHITE)
    wall(1, lo[1], WHITE)
    wall(1, hi[1], WHITE)
    # the end walls are one quad laid down ten times: coincident triangles no split separates, so each half is a
    # big leaf (10 > 8) and the mirror holds pair, quad and unit records -- what the lean kernel needs
    wall(2, lo[2], WHITE, 10)
    wall(2, hi[2], WHITE, 10)
    q.append(("quad", (-5.0, 5.9, 2.0), (5.0, 5.9, 2.0), (5.0, 5.9, 14.0), (-5.0, 5.9, 14.0), LIGHT))
    for i in range(12):
        c, r = room_sphere(i)
        q.append(("sphere", c, r, 3 + i))
    return q


ROOM_SIZE = (53, 29)  # 1537 pixels: each grid sphere covers some 38 of them
DEFAULT_CAMERA = ((0.0, 0.0, 0.0), 0.0, 180.0)  # looks along +z


def room(name, camera=DEFAULT_CAMERA, sky=False, right_wall=True, **expect):
    expect.setdefault("lean", True)
    return case(name, room_materials(), room_prims(right_wall), camera, sky, ROOM_SIZE, **expect)


# ------------------------------------------------------------------------------------------------------
# an open box in the manner of a Cornell box (no mesh in it): five walls, a ceiling light, three spheres
# ------------------------------------------------------------------------------------------------------
def box_case(name, camera, **expect):
    m = [mat(albedo=(0.7, 0.7, 0.7)), mat(albedo=(0.1, 0.7, 0.1)), mat(albedo=(0.7, 0.1, 0.1)),
         mat(emissive=(20.0, 18.0, 14.0)),
         mat(albedo=(0.9, 0.9, 0.5), specular=(0.9, 0.9, 0.9, 0.0), specular_percent=0.5, roughness=0.2),
         mat(albedo=(0.0, 0.0, 1.0), specular=(1.0, 0.0, 0.0, 0.0), specular_percent=0.5, roughness=0.4),
         mat(albedo=(1.0, 1.0, 1.0), specular=(0.3, 1.0, 0.3, 0.0), specular_percent=1.0, roughness=0.0)]
    x, y, z0, z1 = 10.0, 10.0, 12.0, 24.0
    p = [("quad", (-x, -y, z1), (x, -y, z1), (x, y, z1), (-x, y, z1), 0)] * 10  # back wall: the big leaves
    p += [("quad", (-x, -y, z1), (x, -y, z1), (x, -y, z0), (-x, -y, z0), 0),
          ("quad", (-x, y, z1), (x, y, z1), (x, y, z0), (-x, y, z0), 0),
          ("quad", (-x, -y, z1), (-x, -y, z0), (-x, y, z0), (-x, y, z1), 1),
          ("quad", (x, -y, z1), (x, -y, z0), (x, y, z0), (x, y, z1), 2),
          ("quad", (-6.0, y - 0.1, 22.0), (6.0, y - 0.1, 22.0), (6.0, y - 0.1, 14.0), (-6.0, y - 0.1, 14.0), 3),
          ("sphere", (-6.0, -7.0, 18.0), 3.0, 4), ("sphere", (1.0, -7.0, 17.0), 3.0, 5), ("sphere", (6.0, 1.0, 19.0), 3.0, 6)]
    expect.setdefault("lean", True)
    return case(name, m, p, camera, True, ROOM_SIZE, **expect)


# ------------------------------------------------------------------------------------------------------
# the deck: a BVH exactly as deep as asked
# ------------------------------------------------------------------------------------------------------
DECK_TRI = ((-0.3, -0.3, -1.0), (0.3, -0.3, -1.0), (0.0, 0.3, -0.7))  # triangle 0 before its scale
DECK_CAMERA = ((0.0, 0.0, 0.0), 0.0, 0.0)  # at the deck's apex, looking along -z through every triangle


def deck(name, count, top_exp, big_floor=True, **expect):
    """`count` triangles, triangle k = DECK_TRI scaled by 2^(top_exp - k) about the origin (exact in fp32).  All
    centroids have x = 0, so no x split separates them; in z the largest triangle of a node lies alone below the
    midpoint (its centroid at -0.9 of the node's extent, the next at -0.45), so every split peels it into the left
    leaf and the rest goes right: the deck alone is a chain of depth count - 1, whose nested boxes every ray from
    the apex inside the pyramid |x| <= 0.6 |z|, -0.5 |z| <= y <= 0.45 |z| enters one after the other.  The floor
    (ten coincident quads when big_floor: big leaves) and the light have z < 0 too: they leave the chain to the
    left, a few levels down, and add the levels `expect["depth"]` accounts for."""
    m = [mat(albedo=(0.7, 0.7, 0.7)), mat(emissive=(8.0, 8.0, 8.0)),
         mat(albedo=(0.9, 0.5, 0.2), specular=(0.9, 0.9, 0.9, 0.0), specular_percent=0.4, roughness=0.3),
         mat(albedo=(0.2, 0.4, 0.9), specular=(0.9, 0.9, 0.9, 0.0), specular_percent=0.8, roughness=0.1)]
    p = []
    for k in range(count):
        s = 2.0 ** (top_exp - k)
        p.append(("tri", *[tuple(c * s for c in v) for v in DECK_TRI], 2))
    p += [("quad", (-9.0, -3.0, -1.5), (9.0, -3.0, -1.5), (9.0, -3.0, -15.0), (-9.0, -3.0, -15.0), 0)] * (10 if big_floor else 1)
    p.append(("quad", (-4.0, 6.0, -3.0), (4.0, 6.0, -3.0), (4.0, 6.0, -9.0), (-4.0, 6.0, -9.0), 1))
    p.append(("sphere", (5.0, -1.0, -6.0), 2.0, 3))
    expect.setdefault("lean", big_floor)
    return case(name, m, p, DECK_CAMERA, True, ROOM_SIZE, **expect)


def many_spheres():
    """70 spheres (more than the 64 one wave holds) in a 10 x 7 grid on a floor, five materials in turn."""
    m = [mat(albedo=(0.7, 0.7, 0.7)), mat(emissive=(5.0, 5.0, 5.0)),
         mat(albedo=(0.9, 0.3, 0.3)),
         mat(albedo=(0.3, 0.9, 0.3), specular=(0.9, 0.9, 0.9, 0.0), specular_percent=0.5, roughness=0.1),
         mat(albedo=(0.3, 0.3, 0.9), specular=(1.0, 0.8, 0.2, 0.0), specular_percent=1.0, roughness=0.0),
         mat(albedo=(1.2, 1.2, 0.4)),
         mat(albedo=(0.0, 0.0, 0.0), emissive=(1.0, 2.0, 3.0))]
    p = [("quad", (-14.0, -4.0, 4.0), (14.0, -4.0, 4.0), (14.0, -4.0, 30.0), (-14.0, -4.0, 30.0), 0)] * 10
    p.append(("quad", (-6.0, 9.0, 8.0), (6.0, 9.0, 8.0), (6.0, 9.0, 20.0), (-6.0, 9.0, 20.0), 1))
    for i in range(70):
        p.append(("sphere", (-9.9 + 2.2 * (i % 10), -3.0 + 1.9 * (i // 10), 12.0 + 0.7 * (i % 3)), 0.9, 2 + i % 5))
    return case("spheres70", m, p, DEFAULT_CAMERA, True, ROOM_SIZE, lean=True)


INSIDE = 5  # the room sphere the inside-a-sphere pose sits in
_c, _r = room_sphere(INSIDE)
DECK_DEPTHS = (26, 27, 28, 29, 38, 39, 48, 49, 62)  # either side of every stack boundary, and the deepest allowed
REFUSED_DEPTHS = (63, 80)

# a deck of `d` triangles with the floor and the light is d levels deep (asserted by the CPU tests); its scales run
# from 2^((d + 1) // 2) down, inside the mirror's filtered range 2^-60 .. 2^62 for every depth here
CASES = [
    room("room_closed"),
    room("room_open_sky", sky=True, right_wall=False),
    room("room_open_nosky", sky=False, right_wall=False),
    # cameras
    room("room_tilted", camera=((1.5, -1.0, 2.0), 37.0, 211.0), right_wall=False, sky=True, seen=[0, 2, 9, 12]),
    room("room_down_axis", camera=((0.0, 2.0, 8.0), 90.0, 180.0), seen=[0]),
    room("room_inside_sphere", camera=((_c[0] + 0.3, _c[1] - 0.2, _c[2] + 0.1), 0.0, 180.0), seen=[3 + INSIDE], inside=INSIDE),
    # on the red wall's plane, looking into the room: the wall itself is hit at distance 0 by every ray
    room("room_on_wall", camera=((ROOM_LO[0], 0.5, 6.0), 0.0, 270.0), seen=[1]),
    box_case("box_front", ((0.0, 0.0, 5.0), 0.0, 180.0)),
    box_case("box_tilted", ((-9.0, 6.0, -2.0), 37.0, 211.0), seen=[0]),
    box_case("box_all_sky", ((0.0, 0.0, -30.0), 0.0, 0.0), seen=[], hits=0),
    many_spheres(),
] + [deck(f"deck{d}", d, (d + 1) // 2, depth=d) for d in DECK_DEPTHS] + [
    deck("deck29_plain", 29, 15, big_floor=False, depth=29),  # no big leaves: MODE 17 general by default
    # scales 2^-35 .. 2^-62: bounds below 2^-60, the mirror's `fast` flag is 0 and every lane takes the IEEE slab; no
    # deck triangle is large enough to be hit (glm's determinant epsilon), the chain is still walked
    deck("deck30_tiny", 28, -35, depth=30, fast=0, seen=[0, 1, 3]),
]
REFUSED = [deck(f"deck{d}", d, (d + 1) // 2, depth=d, refused=True) for d in REFUSED_DEPTHS]
BY_NAME = {c["name"]: c for c in CASES + REFUSED}
assert len(BY_NAME) == len(CASES) + len(REFUSED)


# ------------------------------------------------------------------------------------------------------
# the oracle's frames of a case, rendered once per process and shared (never modified by a test)
# ------------------------------------------------------------------------------------------------------
_FRAMES = {}


def oracle_frames(case):
    """{"frames": [FRAMES arrays [h, w, 4]], "rng": final states [h * w, 6] uint32, "pending": per pixel, the largest
    number of pending DFS entries over frame 0's rays, "stats": frame 0's OStats, "arrays", "camera"}."""
    got = _FRAMES.get(case["name"])
    if got is None:
        o, code = apply_oracle(case)
        assert code == 0, f"{case['name']}: the oracle's builder refused the scene ({code})"
        w, h = case["width"], case["height"]
        rng = T.oracle_rng_frame(T.SEED, w, h)
        frames, last, pending, stats = [], None, None, None
        for f in range(FRAMES):
            if f == 0:
                img, stats, pending = o.render_pending(w, h, case["spp"], case["bounces"], frame_index=0, rng=rng)
            else:
                img = o.render(w, h, case["spp"], case["bounces"], frame_index=f, rng=rng, last=last)
            frames.append(img)
            last = img
        got = {"frames": frames, "rng": rng, "pending": pending, "stats": stats, "arrays": o.arrays(), "camera": o.camera(w, h)}
        _FRAMES[case["name"]] = got
    return got
