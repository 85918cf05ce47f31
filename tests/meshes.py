"""Synthetic OBJ text for the mesh tests (the reference's skull2.obj lives on the
author's disk only, kernel.cu:1706)."""
import math


def uv_sphere_obj(cx=4.0, cy=2.0, cz=5.0, r=1.6, n_lat=10, n_lon=16, quads=True):
    """Lat/long sphere with v / vt / vn and f a/b/c faces: triangles at the poles,
    quads (or two triangles) elsewhere."""
    lines = ["# synthetic uv sphere"]
    idx = {}
    k = 0
    for i in range(n_lat + 1):
        th = math.pi * i / n_lat
        for j in range(n_lon + 1):
            ph = 2 * math.pi * j / n_lon
            nx, ny, nz = math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph)
            lines.append("v %.6f %.6f %.6f" % (cx + r * nx, cy + r * ny, cz + r * nz))
            lines.append("vt %.6f %.6f" % (j / n_lon, i / n_lat))
            lines.append("vn %.6f %.6f %.6f" % (nx, ny, nz))
            k += 1
            idx[(i, j)] = k
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = idx[(i, j)], idx[(i + 1, j)], idx[(i + 1, j + 1)], idx[(i, j + 1)]
            t = lambda v: "%d/%d/%d" % (v, v, v)
            if i == 0:
                lines.append("f %s %s %s" % (t(a), t(b), t(c)))
            elif i == n_lat - 1:
                lines.append("f %s %s %s" % (t(a), t(b), t(d)))
            elif quads:
                lines.append("f %s %s %s %s" % (t(a), t(b), t(c), t(d)))
            else:
                lines.append("f %s %s %s" % (t(a), t(b), t(c)))
                lines.append("f %s %s %s" % (t(a), t(c), t(d)))
    return "\n".join(lines) + "\n"


FAN_SIZES = (150, 63, 127, 64, 126, 70, 5, 1)


def fan_hub(k, x0=0.0, y0=0.0, z0=6.0, pitch=1.6, dz=0.45):
    """Hub of fan k: a 3-wide grid in x and y, every fan a step farther in z. The first six take their places down
    the columns of the first two rows: that is the order in which the loader's cuts (y, x, z, ...) leave them, so
    leaf k is fan k (asserted on the CPU, tests/test_mesh_large_cpu.py)."""
    slot = (k % 2) * 3 + k // 2 if k < 6 else k
    return (x0 + pitch * (slot % 3), y0 + pitch * (slot // 3), z0 + dz * k)


def fans_obj(sizes=FAN_SIZES, normals=False, rim=0.7, **grid):
    """One triangle fan per entry of `sizes`, every triangle (hub, rim i, rim i + 1): the loader's split sorts
    triangles by their FIRST vertex, so a fan is never cut and becomes one leaf of exactly its length, the triangles
    in the order written. The fans face -z (hub raised towards the viewer: a shallow cone) and their rims wave and zigzag
    in z, so that no two neighbouring triangles are coplanar. Every run of 63 triangles -- what a tile takes at a time --
    shares an equal part of the circle among its members (a member's part at most a sixth before the parts are
    scaled to the whole): the one triangle at position 63 of a fan of 64, or 126 of 127, is wide and shows in a
    small frame. `normals`: vn lines and a//c faces (per-vertex normals, no vt)."""
    lines = ["# triangle fans of %s" % (list(sizes),)]
    faces = []
    nv = nn = 0
    for k, n in enumerate(sizes):
        hx, hy, hz = fan_hub(k, **grid)
        chunks = (n + 62) // 63
        wts = [min(1.0 / (chunks * min(63, n - i // 63 * 63)), 1.0 / 6) for i in range(n)]
        span = 2 * math.pi * (1.0 if n >= 3 else n / 3.0)
        lines.append("v %.6f %.6f %.6f" % (hx, hy, hz - 0.25))
        hub = nv = nv + 1
        first = nv + 1
        acc = 0.0
        for i in range(n + 1):
            th = span * acc / sum(wts) + 0.3 * k
            r = rim * (1 + 0.06 * math.sin(5 * th))
            step = span * wts[min(i, n - 1)] / sum(wts)
            zig = 0.05 * rim * step * (1 if i % 2 else -1)     # a crease at every spoke, whatever the waves do there
            lines.append("v %.6f %.6f %.6f" % (hx + r * math.cos(th), hy + r * math.sin(th),
                                               hz + 0.09 * math.sin(7 * th + k) + 0.04 * math.cos(31 * th) + zig))
            nv += 1
            acc += wts[i] if i < n else 0
        if normals:
            # the hub's normal and one per rim vertex, leaning outwards: interpolated normals differ across a triangle
            lines.append("vn 0 0 -1")
            nn += 1
            hub_n = nn
            for i in range(n + 1):
                th = span * i / max(n, 1)
                lines.append("vn %.6f %.6f %.6f" % (0.5 * math.cos(th), 0.5 * math.sin(th), -1.0))
                nn += 1
            for i in range(n):
                faces.append("f %d//%d %d//%d %d//%d" % (hub, hub_n, first + i, hub_n + 1 + i, first + i + 1, hub_n + 2 + i))
        else:
            faces += ["f %d %d %d" % (hub, first + i, first + i + 1) for i in range(n)]
    return "\n".join(lines + faces) + "\n"


def box_obj_no_normals(x0=1.0, y0=0.0, z0=6.0, s=1.5):
    """A box as 12 bare-index triangles (no vn / vt): the loader's third branch."""
    v = [(x0, y0, z0), (x0 + s, y0, z0), (x0 + s, y0 + s, z0), (x0, y0 + s, z0),
         (x0, y0, z0 + s), (x0 + s, y0, z0 + s), (x0 + s, y0 + s, z0 + s), (x0, y0 + s, z0 + s)]
    f = [(1, 3, 2), (1, 4, 3), (5, 6, 7), (5, 7, 8), (1, 2, 6), (1, 6, 5), (4, 7, 3), (4, 8, 7), (1, 5, 8), (1, 8, 4),
         (2, 3, 7), (2, 7, 6)]
    lines = ["v %.6f %.6f %.6f" % p for p in v] + ["f %d %d %d" % t for t in f]
    return "\n".join(lines) + "\n"


def normals_only_obj():
    """vn but no vt, faces a//c, one quad: the loader's second branch."""
    lines = ["v 2 1 4", "v 5 1 4", "v 5 4 4.5", "v 2 4 4.5", "v 3.5 5.5 4.2",
             "vn 0 0 1", "vn 0 0.1 1", "vn 0.1 0 1",
             "f 1//1 2//2 3//3 4//1", "f 4//1 3//2 5//3"]
    return "\n".join(lines) + "\n"
