"""Writes the textured test scene of this directory (texbox.obj, texbox.mtl, the
untextured twin texbox_twin.obj / .mtl and the PPM maps). The files are committed;
this script documents how they were authored and regenerates them byte for byte.

A closed room x, y in [-2, 2], z in [-2, 4] with one area light under the ceiling:
  back wall   illum 7 (diffuse)  map_Kd wall.ppm 5x3, UVs from -1.5 to 2.3 (wrap, below -1)
  floor       illum 2 (Phong)    map_Kd floor.ppm 4x4, maxval 100
  cube        illum 8 (mixture)  map_Kd cube_kd.ppm 2x3 and map_Ks cube_ks.ppm 3x2 (an option
                                 and a .png name on the line; relative `f` indices)
  left, right, ceiling, front wall: untextured diffuse (faces without vt), light: emitter
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def ppm(name, w, h, maxval, pixel):
    """pixel(x, y) -> (r, g, b) bytes, row 0 = the file's first row (the image's top)."""
    body = bytearray()
    for y in range(h):
        for x in range(w):
            body += bytes(pixel(x, y))
    with open(os.path.join(HERE, name), "wb") as f:
        f.write(b"P6\n%d %d\n%d\n" % (w, h, maxval) + bytes(body))


def main():
    ppm("wall.ppm", 5, 3, 255, lambda x, y: ((40 + 50 * x) % 256, (220 - 90 * y) % 256, (30 + 45 * (x + 2 * y)) % 256))
    ppm("floor.ppm", 4, 4, 100, lambda x, y: (90, 85, 20) if (x + y) % 2 else (15, 30, 95))
    ppm("cube_kd.ppm", 2, 3, 255, lambda x, y: (230 - 100 * y, 40 + 90 * x, 60 + 80 * y))
    ppm("cube_ks.ppm", 3, 2, 255, lambda x, y: (30 + 60 * x, 150 - 100 * y, 90))

    v, vt, vn, body = [], [], [], []

    def quad(name, mtl, p, n, uv=None):
        """p: 4 corners counter-clockwise seen from the side n points to."""
        body.append(f"o {name}\nusemtl {mtl}")
        v.extend(p)
        vn.append(n)
        if uv:
            vt.extend(uv)
            body.append("f " + " ".join(f"{len(v) - 3 + k}/{len(vt) - 3 + k}/{len(vn)}" for k in range(4)))
        else:
            body.append("f " + " ".join(f"{len(v) - 3 + k}//{len(vn)}" for k in range(4)))

    quad("back", "wall_tex", [(-2, -2, -2), (2, -2, -2), (2, 2, -2), (-2, 2, -2)], (0, 0, 1),
         [(-1.5, -1.25), (2.3, -1.25), (2.3, 1.6), (-1.5, 1.6)])
    quad("floor", "floor_phong", [(-2, -2, 4), (2, -2, 4), (2, -2, -2), (-2, -2, -2)], (0, 1, 0),
         [(0, 0), (1.5, 0), (1.5, 2.25), (0, 2.25)])
    quad("left", "red", [(-2, -2, 4), (-2, -2, -2), (-2, 2, -2), (-2, 2, 4)], (1, 0, 0))
    quad("right", "green", [(2, -2, -2), (2, -2, 4), (2, 2, 4), (2, 2, -2)], (-1, 0, 0))
    quad("ceiling", "white", [(-2, 2, -2), (2, 2, -2), (2, 2, 4), (-2, 2, 4)], (0, -1, 0))
    quad("front", "white", [(2, -2, 4), (-2, -2, 4), (-2, 2, 4), (2, 2, 4)], (0, 0, -1))
    quad("light", "lamp", [(-0.6, 1.95, -0.2), (0.6, 1.95, -0.2), (0.6, 1.95, 1.0), (-0.6, 1.95, 1.0)], (0, -1, 0))
    # the cube: x in [-0.9, 0.3], y in [-2, -0.6], z in [-1.0, 0.2], rotated a little, relative indices
    import math
    c, s = math.cos(0.5), math.sin(0.5)
    rot = lambda x, y, z: (round(c * (x + 0.3) - s * (z + 0.4) - 0.3, 6), y, round(s * (x + 0.3) + c * (z + 0.4) - 0.4, 6))
    x0, x1, y0, y1, z0, z1 = -0.9, 0.3, -2.0, -0.6, -1.0, 0.2
    faces = [
        ([(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], (0, 0, 1)),
        ([(x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0)], (0, 0, -1)),
        ([(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)], (-1, 0, 0)),
        ([(x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1)], (1, 0, 0)),
        ([(x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0)], (0, 1, 0)),
        ([(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)], (0, -1, 0)),
    ]
    cube = ["o cube\nusemtl cube_mix"]
    for k, (p, n) in enumerate(faces):
        cube += [f"v {a:g} {b:g} {cc:g}" for a, b, cc in (rot(*q) for q in p)]
        nn = rot(n[0] - 0.3, 0, n[2] - 0.4)
        cube.append(f"vn {nn[0] + 0.3:g} {n[1]:g} {nn[2] + 0.4:g}")
        cube += [f"vt {a:g} {b:g}" for a, b in [(0.1 * k, -0.3), (0.1 * k + 1.2, -0.3), (0.1 * k + 1.2, 0.9), (0.1 * k, 0.9)]]
        cube.append("f -4/-4/-1 -3/-3/-1 -2/-2/-1 -1/-1/-1")

    def obj(mtl):
        return "\n".join([f"# authored by make_scene.py\nmtllib {mtl}"] + [f"v {a:g} {b:g} {c_:g}" for a, b, c_ in v] +
                         [f"vt {a:g} {b:g}" for a, b in vt] + [f"vn {a:g} {b:g} {c_:g}" for a, b, c_ in vn] +
                         body + cube) + "\n"

    mtl = """# authored by make_scene.py
newmtl wall_tex
illum 7
Kd 0.5 0.5 0.5
map_Kd wall.ppm

newmtl floor_phong
illum 2
Kd 0.4 0.4 0.4
Ks 0.3 0.3 0.3
Ns 20
map_Kd floor.ppm

newmtl cube_mix
illum 8
Kd 0.6 0.6 0.6
Ks 0.2 0.2 0.2
Ns 10
map_Kd -clamp on cube_kd.png
map_Ks cube_ks.ppm

newmtl red
illum 7
Kd 0.63 0.065 0.05

newmtl green
illum 7
Kd 0.14 0.45 0.091

newmtl white
illum 7
Kd 0.725 0.71 0.68

newmtl lamp
illum 7
Kd 0 0 0
Ke 17 12 4
"""
    with open(os.path.join(HERE, "texbox.obj"), "w") as f:
        f.write(obj("texbox.mtl"))
    with open(os.path.join(HERE, "texbox_twin.obj"), "w") as f:
        f.write(obj("texbox_twin.mtl"))
    with open(os.path.join(HERE, "texbox.mtl"), "w") as f:
        f.write(mtl)
    with open(os.path.join(HERE, "texbox_twin.mtl"), "w") as f:
        f.write("".join(line + "\n" for line in mtl.splitlines() if not line.startswith("map_")))


CAMERA = dict(eye=(0.3, 0.2, 3.6), at=(-0.2, -0.5, -2.0), up=(0.0, 1.0, 0.0), fov=50.0)

if __name__ == "__main__":
    main()
