"""The composed castRay / castLightRay / rayTrace reference the ray-query tests compare with.

numpy binary32 arrays (numpy has no FMA: every product and sum is rounded as the reference's expressions are) for the
intersections of many rays with one primitive at a time, in castRay's order (mesh leaves behind their own boxes, then
spheres, cubes, planes; strict `t < nt`), plus the oracle's unit entry points for what is not restated: atan2f / acosf
of the texture coordinates and the sky, castLightRay's sample directions, the pack. The primitive restatements are
checked against oracle_sphere/cube/plane/triangle_intersect and the whole reference against oracle_render
(tests/test_query_cpu.py) before any device result is compared with it."""
import ctypes as C

import numpy as np

from test_reflect_cpu import f2i, intersect, normalise, sphere_table

f32 = np.float32
EPS_MT = f32(0.0000001)


def _minm(a, b):   # the reference's min / max macros (kernel.cu:16-26), NaN behaviour included
    return np.where(a < b, a, b)


def _maxm(a, b):
    return np.where(a > b, a, b)


def slab(lo, hi, O, inv):
    """cube::intersect (kernel.cu:457-485) of rays O with inv = 1.f / Dir against the box [lo, hi] -> hit, t."""
    with np.errstate(all="ignore"):
        t1, t2 = (lo[0] - O[:, 0]) * inv[:, 0], (hi[0] - O[:, 0]) * inv[:, 0]
        t3, t4 = (lo[1] - O[:, 1]) * inv[:, 1], (hi[1] - O[:, 1]) * inv[:, 1]
        t5, t6 = (lo[2] - O[:, 2]) * inv[:, 2], (hi[2] - O[:, 2]) * inv[:, 2]
    tmin = _maxm(_maxm(_minm(t1, t2), _minm(t3, t4)), _minm(t5, t6))
    tmax = _minm(_minm(_maxm(t1, t2), _maxm(t3, t4)), _maxm(t5, t6))
    hit = ~(tmax < 0) & ~(tmax < tmin)
    return hit, np.where(hit, tmin, tmax).astype(np.float32)


def plane_hit(p, n, O, D):
    """plane::intersect (kernel.cu:370-380), p the point and n the normal as stored."""
    with np.errstate(all="ignore"):
        denom = (n[0] * D[:, 0] + n[1] * D[:, 1]) + n[2] * D[:, 2]
        pl = (p[None, :] - O).astype(np.float32)
        t = (((pl[:, 0] * n[0] + pl[:, 1] * n[1]) + pl[:, 2] * n[2]) / denom).astype(np.float32)
    return (denom < 0) & (t >= 0), t


def tri_hit(p0, p1, p2, O, D):
    """mesh::rayIntersect (Moller-Trumbore, kernel.cu:1024-1059) -> hit, t, u, v."""
    with np.errstate(all="ignore"):
        e1, e2 = (p1 - p0).astype(np.float32), (p2 - p0).astype(np.float32)
        h = np.stack([D[:, 1] * e2[2] - D[:, 2] * e2[1], D[:, 2] * e2[0] - D[:, 0] * e2[2],
                      D[:, 0] * e2[1] - D[:, 1] * e2[0]], axis=1).astype(np.float32)
        a = (e1[0] * h[:, 0] + e1[1] * h[:, 1]) + e1[2] * h[:, 2]
        f = (f32(1) / a).astype(np.float32)
        s = (O - p0[None, :]).astype(np.float32)
        u = (f * ((s[:, 0] * h[:, 0] + s[:, 1] * h[:, 1]) + s[:, 2] * h[:, 2])).astype(np.float32)
        q = np.stack([s[:, 1] * e1[2] - s[:, 2] * e1[1], s[:, 2] * e1[0] - s[:, 0] * e1[2],
                      s[:, 0] * e1[1] - s[:, 1] * e1[0]], axis=1).astype(np.float32)
        v = (f * ((D[:, 0] * q[:, 0] + D[:, 1] * q[:, 1]) + D[:, 2] * q[:, 2])).astype(np.float32)
        t = (f * ((e2[0] * q[:, 0] + e2[1] * q[:, 1]) + e2[2] * q[:, 2])).astype(np.float32)
        rej = ((a > -EPS_MT) & (a < EPS_MT)) | (u < 0) | (u > 1) | (v < 0) | ((u + v) > 1)
    return ~rej & (t >= EPS_MT), t, u, v


def _vec(v):
    return np.array([v.x, v.y, v.z], dtype=np.float32)


class CastRef:
    """castRay / castLightRay / rayTrace over a scene's inputs (tests/scenes.py Inputs, plus planes, cubes, a mesh)."""

    def __init__(self, oracle, inp, mesh_text=None, spheres=True):
        self.oracle = oracle
        self.lib = oracle.load()
        self.n = inp.n if spheres else 0
        self.tab = sphere_table(inp.spheres, inp.n)[: self.n]
        self.planes = [(_vec(inp.planes[i].orgin), _vec(inp.planes[i].normal)) for i in range(getattr(inp, "n_planes", 0))]
        self.cubes = [(_vec(inp.cubes[i].bounds[0]), _vec(inp.cubes[i].bounds[1]), _vec(inp.cubes[i].orgin))
                      for i in range(getattr(inp, "n_cubes", 0))]
        self.tex = [np.ascontiguousarray(p, dtype=np.float32) for p in inp.tex]
        self.sky = [np.ascontiguousarray(p, dtype=np.float32) for p in inp.sky]
        self.sky_c = _vec(inp.sky_box.orgin)
        self.sky_w = f32(inp.sky_box.radius) * f32(inp.sky_box.radius)
        self.lights, self.n_lights = inp.lights, inp.n_lights
        self.olights = C.cast(inp.lights, C.POINTER(oracle.OLight))
        self.tris, self.boxes, self.mesh_normals = [], [], False
        if mesh_text is not None:
            self.mesh = oracle.Mesh(mesh_text)
            tp = self.lib.oracle_mesh_triangles(self.mesh.handle)
            for i in range(self.mesh.poly_count):
                t = tp[i]
                self.tris.append({"p": [_vec(t.points[k]) for k in range(3)], "n": _vec(t.normal),
                                  "vn": [_vec(t.vecNormal[k]) for k in range(3)],
                                  "vt": np.array([[t.vt[k][0], t.vt[k][1]] for k in range(3)], dtype=np.float32)})
            for j in range(self.mesh.bvhbox_count):
                bounds, orgin = (C.c_float * 6)(), (C.c_float * 3)()
                idx, cnt = C.POINTER(C.c_int)(), C.c_int()
                assert self.lib.oracle_mesh_box(self.mesh.handle, j, bounds, orgin, C.byref(idx), C.byref(cnt)) == 0
                self.boxes.append((np.array(bounds[:3], dtype=np.float32), np.array(bounds[3:], dtype=np.float32),
                                   [idx[i] for i in range(cnt.value)]))
            self.mesh_normals = self.mesh.has_normals

    # ------------------------------------------------------------------ castRay
    def nearest(self, O, D):
        """castRay (kernel.cu:1287-1431) -> dict of t, kind, index, u, v, tx, ty, normal, new_org (rt_hit's fields)
        and `gated`: rays that pass through a triangle their leaf's box test hides."""
        m = O.shape[0]
        nt = np.full(m, np.inf, dtype=np.float32)
        kind = np.full(m, -1, dtype=np.int32)
        index = np.full(m, -1, dtype=np.int32)
        uu = np.zeros(m, dtype=np.float32)
        vv = np.zeros(m, dtype=np.float32)
        gated = np.zeros(m, dtype=bool)
        with np.errstate(all="ignore"):
            inv = (f32(1) / D).astype(np.float32)
        for lo, hi, members in self.boxes:
            gate, _ = slab(lo, hi, O, inv)
            for ti in members:
                p = self.tris[ti]["p"]
                h, t, u, v = tri_hit(p[0], p[1], p[2], O, D)
                gated |= h & ~gate
                w = h & gate & (t < nt)
                nt[w], kind[w], index[w], uu[w], vv[w] = t[w], 0, ti, u[w], v[w]
        for i in range(self.n):
            h, t = intersect(O, D, self.tab[i:i + 1])
            w = h[:, 0] & (t[:, 0] < nt)
            nt[w], kind[w], index[w], uu[w], vv[w] = t[w, 0], 1, i, 0, 0
        for i, (lo, hi, _) in enumerate(self.cubes):
            h, t = slab(lo, hi, O, inv)
            w = h & (t < nt)
            nt[w], kind[w], index[w], uu[w], vv[w] = t[w], 3, i, 0, 0
        for i, (p, n) in enumerate(self.planes):
            h, t = plane_hit(p, n, O, D)
            w = h & (t < nt)
            nt[w], kind[w], index[w], uu[w], vv[w] = t[w], 2, i, 0, 0
        miss = nt == np.inf
        kind[miss], index[miss] = -1, -1
        rec = {"t": nt, "kind": kind, "index": index, "u": uu, "v": vv, "gated": gated,
               "tx": np.zeros(m, dtype=np.float32), "ty": np.zeros(m, dtype=np.float32),
               "normal": np.zeros((m, 3), dtype=np.float32), "new_org": np.zeros((m, 3), dtype=np.float32)}
        for i in np.nonzero(~miss)[0]:
            self._record(rec, i, O[i], D[i])
        return rec

    def _record(self, rec, i, o, d):
        """The hit record of kernel.cu:1376-1426 for ray i."""
        t, k, j = rec["t"][i], rec["kind"][i], rec["index"][i]
        with np.errstate(all="ignore"):
            hp = (o + d * t).astype(np.float32)
        tx = ty = f32(0.5)
        if k == 0:
            tr = self.tris[j]
            u, v = rec["u"][i], rec["v"][i]
            w0 = f32(f32(1) - u) - v
            if self.mesh_normals:
                vn = tr["vn"]
                nrm = ((vn[0] * w0 + vn[1] * u) + vn[2] * v).astype(np.float32)
                nrm = normalise(nrm[None, :])[0]
            else:
                nrm = tr["n"].copy()
            vt = tr["vt"]
            tx = f32(f32(f32(w0 * vt[0, 0]) + f32(u * vt[1, 0])) + f32(v * vt[2, 0]))
            ty = f32(f32(f32(w0 * vt[0, 1]) + f32(u * vt[1, 1])) + f32(v * vt[2, 1]))
            new_org = (nrm + hp).astype(np.float32)
        elif k == 2:
            nrm, new_org = self.planes[j][1].copy(), hp
        else:
            c = self.tab[j, :3] if k == 1 else self.cubes[j][2]
            nrm = normalise((hp - c).astype(np.float32)[None, :])[0]
            tx = f32((1.0 + float(f32(self.lib.oracle_atan2f(float(nrm[2]), float(nrm[0])))) / 3.1415) * 0.5)
            ty = f32(float(f32(self.lib.oracle_acosf(float(nrm[1])))) / 3.1415)
            new_org = hp
        rec["tx"][i], rec["ty"][i], rec["normal"][i], rec["new_org"][i] = tx, ty, nrm, new_org

    # ------------------------------------------------------------------ castLightRay's any-hit
    def occluded(self, O, D):
        """1 where a triangle (behind its leaf's box), sphere, plane or cube reports a hit (kernel.cu:1475-1536)."""
        m = O.shape[0]
        occ = np.zeros(m, dtype=bool)
        with np.errstate(all="ignore"):
            inv = (f32(1) / D).astype(np.float32)
        for lo, hi, members in self.boxes:
            gate, _ = slab(lo, hi, O, inv)
            for ti in members:
                p = self.tris[ti]["p"]
                occ |= gate & tri_hit(p[0], p[1], p[2], O, D)[0]
        for c0 in range(0, self.n, 256):
            occ |= intersect(O, D, self.tab[c0:c0 + 256])[0].any(axis=1)
        for p, n in self.planes:
            occ |= plane_hit(p, n, O, D)[0]
        for lo, hi, _ in self.cubes:
            occ |= slab(lo, hi, O, inv)[0]
        return occ.astype(np.int32)

    # ------------------------------------------------------------------ rayTrace's pixel body
    def sky_color(self, o, d):
        tab = np.array([[*self.sky_c, self.sky_w]], dtype=np.float32)
        _, t = intersect(o[None, :], d[None, :], tab)
        with np.errstate(all="ignore"):
            hp = (o + d * t[0, 0]).astype(np.float32)
        nrm = normalise((hp - self.sky_c).astype(np.float32)[None, :])[0]
        h, w = self.sky[0].shape
        a = f32(self.lib.oracle_atan2f(float(nrm[2]), float(nrm[0])))
        ix = f2i(f32(f32(f32(f32(1) + f32(a / f32(3.1415))) * f32(0.5)) * f32(w)))
        iy = f2i(f32(f32(f32(self.lib.oracle_acosf(float(nrm[1]))) / f32(3.1415)) * f32(h)))
        idx = int(min(max(int(iy) * w + int(ix), 0), w * h - 1))
        return np.array([self.sky[0].flat[idx], self.sky[1].flat[idx], self.sky[2].flat[idx]], dtype=np.float32)

    def shade(self, O, D):
        """rgba (m, 4) and packed (m,) of rayTrace's pixel body for each ray (kernel.cu:1633-1690)."""
        m = O.shape[0]
        rec = self.nearest(O, D)
        c = np.zeros((m, 3), dtype=np.float32)
        hits = np.nonzero(rec["kind"] >= 0)[0]
        for i in np.nonzero(rec["kind"] < 0)[0]:
            c[i] = self.sky_color(O[i], D[i])
        th, tw = self.tex[0].shape
        oc = self.oracle
        sv = oc.OVec3()
        dirs = np.zeros((len(hits), max(self.n_lights, 1), 10, 3), dtype=np.float32)
        starts = np.zeros((len(hits), 3), dtype=np.float32)
        buf = (C.c_float * 30)()
        for k, i in enumerate(hits):
            nrm, no = rec["normal"][i], rec["new_org"][i]
            starts[k] = (nrm * f32(0.00001) + no).astype(np.float32)
            sv.x, sv.y, sv.z = (float(x) for x in starts[k])
            for li in range(self.n_lights):
                self.lib.oracle_light_dirs(C.byref(sv), C.byref(self.olights[li]), buf)
                dirs[k, li] = np.frombuffer(buf, dtype=np.float32).reshape(10, 3)
        nl = self.n_lights
        if len(hits):
            So = np.repeat(starts, nl * 10, axis=0)
            occ = self.occluded(So, dirs.reshape(-1, 3)).reshape(len(hits), nl, 10)
        for k, i in enumerate(hits):
            ci = int(f2i(f32(rec["ty"][i] * f32(th)))) * tw + int(f2i(f32(rec["tx"][i] * f32(tw))))
            ci = min(max(ci, 0), tw * th - 1)
            texel = (self.tex[0].flat[ci], self.tex[1].flat[ci], self.tex[2].flat[ci])
            nrm = rec["normal"][i]
            acc = [f32(0), f32(0), f32(0)]
            for li in range(nl):
                L = self.lights[li]
                b = f32(0)
                for _ in range(int((occ[k, li] == 0).sum())):
                    b = f32(float(b) + 0.1)                      # b += 0.1 (kernel.cu:1538)
                toL = (np.array([L.pos.x, L.pos.y, L.pos.z], dtype=np.float32) - starts[k]).astype(np.float32)
                for _ in range(21):                              # kernel.cu:1438, then twice per sample (:1465-1466)
                    toL = normalise(toL[None, :])[0]
                a = f32(f32(nrm[0] * toL[0] + nrm[1] * toL[1]) + nrm[2] * toL[2])
                b = f32(b * (a if a > 0 else f32(0)))
                for ch, lc in enumerate((L.r, L.g, L.b)):
                    acc[ch] = f32(acc[ch] + f32(f32(b * f32(lc)) * texel[ch]))
            c[i] = acc
        c = (f32(0) + c).astype(np.float32)
        rgba = np.ones((m, 4), dtype=np.float32)
        rgba[:, :3] = c
        packed = np.array([self.lib.oracle_pack_color(float(x[0]), float(x[1]), float(x[2])) for x in c], dtype=np.uint32)
        return rgba, packed, rec
