"""A float64 model of the surface that gfx_shell_trace intersects, in numpy.  It is a model of the SURFACE, not of the algorithm,
and shares no line with csrc/nrtdsm/:

    S(u, v, h) = P(alpha, beta) + (base + scale * h) * N(alpha, beta)

with (alpha, beta) the barycentrics of (u, v) in a base triangle's texture footprint, P and N the barycentric interpolations of its
vertices (N not renormalised), base = hOffset - scale * hBias, scale = hScale / sqrt(texScale.x texScale.y).  The shell mesh lives
in the unit tile; tile (i, j) holds a copy shifted by (i, j, 0).  A point of shell triangle m in tile (i, j) is
(u, v, h) = m0 + a (m1 - m0) + b (m2 - m0) + (i, j, 0) with the triangle's own barycentrics (a, b).

A ray's closest hit is found in two steps: brute force over flat facets (every (base triangle, tile, shell triangle) whose
footprints overlap, the shell triangle cut k x k, the corners mapped), then Newton's iteration in (a, b, t) on the exact mapped
patch.  Spheres around the facets of one (base triangle, tile) keep the brute force to the pairs that can meet."""
import numpy as np

from tests import tfdm_host as T

EDGE_EPS = 1e-4


class Surface:
    def __init__(self, vertices, triangles, geoms, gp):
        tri = np.asarray(triangles).reshape(-1, 3)
        self.p = vertices["position"][tri].astype(np.float64)            # [T, 3, 3]
        self.n = vertices["normal"][tri].astype(np.float64)
        uv = vertices["texCoord"][tri].astype(np.float64)
        X = T.transform64(gp)
        self.tc = uv @ X[:2, :2].T + X[:2, 2]                              # [T, 3, 2]
        self.base, self.scale = T.height_terms64(gp)
        self.toBc = np.full((len(tri), 3, 3), np.nan)                      # (u, v, 1) -> barycentrics
        for i, t in enumerate(self.tc):
            m = np.stack([t[:, 0], t[:, 1], np.ones(3)])
            if abs(np.linalg.det(m)) > 0:
                self.toBc[i] = np.linalg.inv(m)
        ms, gs = [], []
        for g, (pos, idx) in enumerate(geoms):
            pos = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
            idx = np.asarray(idx).reshape(-1, 3)
            ms.append(pos[idx])
            gs.append(np.full(len(idx), g))
        self.m = np.concatenate(ms)                                        # [M, 3, 3] (u, v, h)
        self.geom = np.concatenate(gs)
        self.hlo, self.hhi = self.m[..., 2].min(), self.m[..., 2].max()
        self.extent = float(np.linalg.norm(self.p.reshape(-1, 3).max(0) - self.p.reshape(-1, 3).min(0)))

    # ---- the map
    def uvh(self, tile, tri, a, b):
        m = self.m[tri]
        out = m[..., 0, :] + a[..., None] * (m[..., 1, :] - m[..., 0, :]) + b[..., None] * (m[..., 2, :] - m[..., 0, :])
        out = out.copy()
        out[..., 0] += tile[..., 0]
        out[..., 1] += tile[..., 1]
        return out

    def at(self, prim, uvh):
        """S, N, w (base barycentrics) of shell-space points on base triangle(s) `prim`."""
        w = np.einsum("...jk,...k->...j", self.toBc[prim], np.concatenate([uvh[..., :2], np.ones(uvh.shape[:-1] + (1,))], -1))
        P = np.einsum("...k,...kc->...c", w, self.p[prim])
        N = np.einsum("...k,...kc->...c", w, self.n[prim])
        return P + (self.base + self.scale * uvh[..., 2])[..., None] * N, N, w

    def point(self, prim, tile, tri, a, b):
        return self.at(prim, self.uvh(tile, tri, a, b))[0]

    def jacobian(self, prim, uvh):
        """d S / d (u, v, h) as [..., 3 (xyz), 3 (u, v, h)]."""
        _, N, _ = self.at(prim, uvh)
        H = self.base + self.scale * uvh[..., 2]
        q = self.p[prim] + H[..., None, None] * self.n[prim]               # [..., 3 (vertex), 3]
        Ju = np.einsum("...k,...kc->...c", self.toBc[prim][..., :, 0], q)
        Jv = np.einsum("...k,...kc->...c", self.toBc[prim][..., :, 1], q)
        return np.stack([Ju, Jv, self.scale * N], -1)

    def patch(self, prim, tile, tri, a, b):
        """S, dS/da, dS/db of the mapped shell triangle."""
        x = self.uvh(tile, tri, a, b)
        J = self.jacobian(prim, x)
        m = self.m[tri]
        return self.at(prim, x)[0], np.einsum("...ck,...k->...c", J, m[..., 1, :] - m[..., 0, :]), np.einsum("...ck,...k->...c", J, m[..., 2, :] - m[..., 0, :])

    def normal(self, prim, tile, tri, a, b):
        """The unit normal dS/da x dS/db, oriented to the side the shell triangle's winding faces in right-handed (u, v, h): the map
        reverses orientation where det dS / d(u, v, h) < 0 (mirrored texture coordinates, or a negative scale)."""
        x = self.uvh(tile, tri, a, b)
        _, SA, SB = self.patch(prim, tile, tri, a, b)
        c = np.cross(SA, SB) * np.sign(np.linalg.det(self.jacobian(prim, x)))[..., None]
        return c / np.linalg.norm(c, axis=-1, keepdims=True)

    # ---- facets
    def candidates(self, ti):
        """[(tile (i, j), shell triangle indices)] whose footprints overlap base triangle ti's (bounds, then separating axes)."""
        tc = self.tc[ti]
        lo, hi = tc.min(0), tc.max(0)
        out = []
        for j in range(int(np.floor(lo[1])), int(np.ceil(hi[1]))):
            for i in range(int(np.floor(lo[0])), int(np.ceil(hi[0]))):
                uv = self.m[..., :2] + np.array([i, j], np.float64)
                mlo, mhi = uv.min(1), uv.max(1)
                keep = (mhi[:, 0] >= lo[0]) & (mlo[:, 0] <= hi[0]) & (mhi[:, 1] >= lo[1]) & (mlo[:, 1] <= hi[1])
                # the base triangle's three edge normals as separating axes
                for k in range(3):
                    e = tc[(k + 1) % 3] - tc[k]
                    ax = np.array([e[1], -e[0]])
                    s, t = uv @ ax, tc @ ax
                    keep &= (s.max(1) >= t.min()) & (s.min(1) <= t.max())
                idx = np.nonzero(keep)[0]
                if len(idx):
                    out.append(((i, j), idx))
        return out

    def facets(self, ti, tile, tris, k):
        """k x k flat facets of the shell triangles `tris` in `tile` on base triangle ti: their (a, b) [F, 3, 2], texture
        coordinates [F, 3, 2], points [F, 3, 3] and shell triangle [F]."""
        cells = []
        for a in range(k):
            for b in range(k - a):
                cells.append(((a, b), (a + 1, b), (a, b + 1)))
                if a + b + 1 < k:
                    cells.append(((a + 1, b), (a + 1, b + 1), (a, b + 1)))
        ab = np.array(cells, np.float64) / k                               # [C, 3, 2]
        fab = np.tile(ab[None], (len(tris), 1, 1, 1)).reshape(-1, 3, 2)
        ftri = np.repeat(tris, len(ab))
        tl = np.broadcast_to(np.array(tile, np.float64), (len(ftri), 3, 2))
        x = self.uvh(tl, ftri[:, None], fab[..., 0], fab[..., 1])
        return fab, x[..., :2], self.at(ti, x)[0], ftri

    def chunks(self, k):
        out = []
        for ti in range(len(self.p)):
            if not np.isfinite(self.toBc[ti]).all():
                continue
            span = (self.tc[ti].max(0) - self.tc[ti].min(0)).max()
            for tile, tris in self.candidates(ti):
                # a shell triangle much larger than the footprint is cut finer: a facet then spans a third of the footprint at most
                # (k = 1 is kept: there the caller says the map is affine)
                size = (self.m[tris][..., :2].max(1) - self.m[tris][..., :2].min(1)).max()
                kk = k if k == 1 else int(min(max(k, np.ceil(3.0 * size / span)), 12))
                fab, ft, fp, ftri = self.facets(ti, tile, tris, kk)
                pts = fp.reshape(-1, 3)
                centre = 0.5 * (pts.min(0) + pts.max(0))
                out.append((ti, tile, fab, ft, fp, ftri, centre, np.linalg.norm(pts - centre, axis=1).max() * 1.1 + 1e-9 * self.extent))
        return out

    # ---- rays
    def trace(self, org, d, tmin, tmax, k=2):
        """Closest hit per ray: dict t (inf: miss), prim, tile [R, 2], tri, a, b, alpha, beta, flagged (the edge rule)."""
        org, d = org.astype(np.float64), d.astype(np.float64)
        tmin, tmax = np.asarray(tmin, np.float64), np.asarray(tmax, np.float64)
        R = len(org)
        best = {"t": np.full(R, np.inf), "prim": np.full(R, -1), "tile": np.zeros((R, 2), np.int64), "tri": np.full(R, -1), "a": np.zeros(R), "b": np.zeros(R)}
        grazing = np.zeros(R, bool)
        ok = np.isfinite(org).all(1) & np.isfinite(d).all(1) & ((d * d).sum(1) > 0)
        dn = np.where(ok[:, None], d, 1.0)
        dn = dn / np.linalg.norm(dn, axis=1, keepdims=True)
        for ti, tile, fab, ft, fp, ftri, centre, radius in self.chunks(k):
            oc = centre - org
            idx = np.nonzero(ok & (np.linalg.norm(oc - (oc * dn).sum(1)[:, None] * dn, axis=1) <= radius))[0]
            if not len(idx):
                continue
            # every facet the ray crosses inside the base triangle is polished: the closest flat facet need not be the closest patch
            clip = (ft[:, 0], ft[:, 1], ft[:, 2], np.broadcast_to(self.tc[ti], (len(ft), 3, 2)), np.zeros(len(ft), np.int64))
            ri, fi, t0, ab0, crossed = _all_hits(fp, org[idx], d[idx], tmin[idx], tmax[idx], clip)
            if not len(ri):
                continue
            ri = idx[ri]
            a0 = fab[fi, 0] + ab0[:, :1] * (fab[fi, 1] - fab[fi, 0]) + ab0[:, 1:] * (fab[fi, 2] - fab[fi, 0])
            tl = np.broadcast_to(np.array(tile, np.float64), (len(ri), 2))
            a, b, tt, good = self._polish(ti, tl, ftri[fi], a0[:, 0], a0[:, 1], t0, org[ri], d[ri])
            np.logical_or.at(grazing, ri[~good & crossed], True)
            good &= (tt > tmin[ri]) & (tt < tmax[ri])
            ri, fi, a, b, tt = ri[good], fi[good], a[good], b[good], tt[good]
            order = np.lexsort((tt, ri))
            ri, fi, a, b, tt = ri[order], fi[order], a[order], b[order], tt[order]
            first = np.ones(len(ri), bool)
            first[1:] = ri[1:] != ri[:-1]
            ri, fi, a, b, tt = ri[first], fi[first], a[first], b[first], tt[first]
            better = (tt < best["t"][ri]) | ((tt == best["t"][ri]) & (ti < best["prim"][ri]))
            r = ri[better]
            best["t"][r], best["prim"][r], best["tri"][r], best["a"][r], best["b"][r] = tt[better], ti, ftri[fi[better]], a[better], b[better]
            best["tile"][r] = tile
        # the edge rule
        h = np.isfinite(best["t"])
        flagged = grazing & ~h                         # a flat facet was crossed, Newton found no root anywhere: the ray grazes
        best["alpha"], best["beta"] = np.zeros(R), np.zeros(R)
        if h.any():
            x = self.uvh(best["tile"][h].astype(np.float64), best["tri"][h], best["a"][h], best["b"][h])
            _, _, w = self.at(best["prim"][h], x)
            best["alpha"][h], best["beta"][h] = w[:, 1], w[:, 2]
            a, b = best["a"][h], best["b"][h]
            fu, fv = x[:, 0] - np.floor(x[:, 0]), x[:, 1] - np.floor(x[:, 1])
            border = np.minimum(np.minimum(fu, 1 - fu), np.minimum(fv, 1 - fv))
            fl = (w.min(1) < EDGE_EPS) | (np.minimum(np.minimum(a, b), 1 - a - b) < EDGE_EPS) | (border < EDGE_EPS)
            flagged[h] = fl
        best["flagged"] = flagged
        return best

    def _polish(self, ti, tile, tri, a, b, t, org, d):
        """Newton in (a, b, t) on the exact mapped patch of shell triangle `tri` in `tile`, from the flat facet's hit."""
        ti = np.broadcast_to(np.asarray(ti), a.shape)
        a, b, t = a.copy(), b.copy(), t.copy()
        with np.errstate(all="ignore"):
            for _ in range(12):
                S, SA, SB = self.patch(ti, tile, tri, a, b)
                F = S - org - t[:, None] * d
                J = np.stack([SA, SB, -d], -1)
                bad = ~np.isfinite(J).all((1, 2)) | (np.abs(np.linalg.det(np.nan_to_num(J))) < 1e-300)
                J[bad] = np.eye(3)
                step = np.linalg.solve(J, F[..., None])[..., 0]
                step[bad] = np.nan
                a, b, t = a - step[:, 0], b - step[:, 1], t - step[:, 2]
            S = self.patch(ti, tile, tri, a, b)[0]
            res = np.linalg.norm(S - org - t[:, None] * d, axis=1)
            fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(t)
            a, b, t = np.where(fin, a, 0.3), np.where(fin, b, 0.3), np.where(fin, t, 0.0)
            _, _, w = self.at(ti, self.uvh(tile, tri, a, b))
            good = fin & (res < 1e-12 * self.extent) & (np.minimum(np.minimum(a, b), 1 - a - b) >= -1e-9) & (w.min(1) >= -1e-9)
        return a, b, t, good


def _all_hits(fp, org, d, tmin, tmax, clip):
    """Every (ray, facet) crossing inside the clip triangle, with a margin: ray index, facet index, t, the facet's own barycentrics
    [n, 2], and whether the flat facet itself is crossed."""
    A, e1, e2 = fp[:, 0], fp[:, 1] - fp[:, 0], fp[:, 2] - fp[:, 0]
    tA, tB, tC, baseTc, _ = clip
    area = T._cross2(baseTc[:, 1] - baseTc[:, 0], baseTc[:, 2] - baseTc[:, 0])
    ri, fi, ts, abs_, cr = [], [], [], [], []
    chunk = max(1, int(2e6 // max(len(A), 1)))
    with np.errstate(all="ignore"):
        for s in range(0, len(org), chunk):
            o, dd = org[s:s + chunk, None, :], d[s:s + chunk, None, :]
            pv = np.cross(dd, e2[None])
            inv = 1.0 / (e1[None] * pv).sum(-1)
            tv = o - A[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            v = (dd * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv
            hp = (1 - u - v)[..., None] * tA[None] + u[..., None] * tB[None] + v[..., None] * tC[None]
            bB = T._cross2(baseTc[None, :, 2] - hp, baseTc[None, :, 0] - hp) / area[None]
            bC = T._cross2(baseTc[None, :, 0] - hp, baseTc[None, :, 1] - hp) / area[None]
            # a margin of a twentieth of the facet: the exact patch bulges from its flat facet, and may be crossed where that is missed
            m = np.minimum(np.minimum(np.minimum(u, v), 1 - u - v), np.minimum(np.minimum(bB, bC), 1 - bB - bC))
            okm = (m >= -0.05) & (t > tmin[s:s + chunk, None] - 1e-3) & (t < tmax[s:s + chunk, None])
            r, f = np.nonzero(okm)
            ri.append(r + s); fi.append(f); ts.append(t[r, f]); abs_.append(np.stack([u[r, f], v[r, f]], 1))
            cr.append((m[r, f] >= 0) & (t[r, f] > tmin[s:s + chunk][r]))
    return np.concatenate(ri), np.concatenate(fi), np.concatenate(ts), np.concatenate(abs_), np.concatenate(cr)
