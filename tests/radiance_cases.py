"""A caller-built scene for rt_radiance's arbitrary-ray test, in the format of tests/scene_cases.py: a box with one
side open, a sphere inside, no sky; every material purely emissive with a colour of its own and zero albedo, so the
radiance of a one-bounce path is exactly the emissive colour of the first hit's material, and 0 on a miss.

ORIGINS: inside the box, in the plane of the opening, and outside in front of it; from each, a panorama sees both
the box and the empty space around it.
"""
import scene_cases as C

LO, HI = (-2.0, -1.5, 3.0), (2.0, 1.5, 7.0)  # the side z = LO[2] is the opening
PANORAMA = (96, 48)
ORIGINS = {"inside": (0.3, -0.2, 5.5), "opening": (0.4, 0.3, 3.0), "outside": (-0.5, 0.4, -2.0)}
COLOURS = [(1.0, 0.25, 0.5), (0.125, 2.0, 0.75), (3.0, 0.5, 0.0625), (0.375, 0.625, 4.0), (1.5, 1.25, 0.875), (0.0, 5.0, 2.5)]


def emissive_box():
    m = [C.mat(albedo=(0.0, 0.0, 0.0), emissive=c) for c in COLOURS]
    (x0, y0, z0), (x1, y1, z1) = LO, HI
    p = [("quad", (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), 0),  # back
         ("quad", (x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), 1),  # left
         ("quad", (x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0), 2),  # right
         ("quad", (x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), 3),  # floor
         ("quad", (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1), 4),  # ceiling
         ("sphere", (-0.8, -0.7, 6.0), 0.6, 5)]
    return C.case("emissive_box", m, p, C.DEFAULT_CAMERA, False, C.ROOM_SIZE, lean=False)


CASE = emissive_box()
