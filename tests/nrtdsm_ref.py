"""A float64 model of the surface that gfx_nrtdsm_trace intersects, in numpy.  It is a model of the SURFACE, not of the algorithm,
and shares no line with csrc/nrtdsm/:

    S(alpha, beta) = P(alpha, beta) + (base + scale * h(tc(alpha, beta))) * N(alpha, beta)

with P, tc, N the barycentric interpolations of a base triangle's vertices (N not renormalised), base = hOffset - scale * hBias,
scale = hScale / sqrt(texScale.x texScale.y), and h the height map's corner samples interpolated affinely over each half texel, the
texel split along its TL-BR diagonal.

A ray's closest hit is found in two steps: brute force over flat facets (every half texel under a base triangle cut into k x k
sub-triangles whose corners lie on S), then Newton's iteration in (alpha, beta, t) on the exact patch of the half texel the
candidate lies in.  Spheres around groups of facets (per base triangle, per 8 x 8 block of texels) keep the brute force to the pairs
that can meet."""
import numpy as np

from tests import tfdm_host as T

TILE = 8


class Surface:
    def __init__(self, vertices, triangles, level0, gp):
        tri = np.asarray(triangles).reshape(-1, 3)
        self.p = vertices["position"][tri].astype(np.float64)            # [T, 3, 3]
        self.n = vertices["normal"][tri].astype(np.float64)
        uv = vertices["texCoord"][tri].astype(np.float64)
        X = T.transform64(gp)
        self.tc = uv @ X[:2, :2].T + X[:2, 2]                              # [T, 3, 2]
        self.base, self.scale = T.height_terms64(gp)
        self.res = level0.shape[0]
        self.corner = T.corner_heights64(level0)                           # [res + 1, res + 1], index [y, x]
        self.extent = float(np.linalg.norm(self.p.reshape(-1, 3).max(0) - self.p.reshape(-1, 3).min(0)))

    # ---- the height function and its pieces
    def piece(self, tc):
        """The half texel `tc` [..., 2] lies in: (h0, gu, gv, u0, v0) with h = h0 + gu (u - u0) + gv (v - v0), u, v in texels;
        and (x, y, upper) identifying it."""
        s = tc * self.res
        x, y = np.floor(s[..., 0]).astype(np.int64), np.floor(s[..., 1]).astype(np.int64)
        fu, fv = s[..., 0] - x, s[..., 1] - y
        n = self.res
        hTL, hTR = self.corner[y % n, x % n], self.corner[y % n, x % n + 1]
        hBL, hBR = self.corner[y % n + 1, x % n], self.corner[y % n + 1, x % n + 1]
        upper = fu >= fv                                                    # TL-BR-TR; else TL-BL-BR
        gu = np.where(upper, hTR - hTL, hBR - hBL)
        gv = np.where(upper, hBR - hTR, hBL - hTL)
        return hTL, gu, gv, x.astype(np.float64), y.astype(np.float64), (x, y, upper), (fu, fv)

    def height(self, tc):
        h0, gu, gv, u0, v0, _, (fu, fv) = self.piece(tc)
        return h0 + gu * fu + gv * fv

    def bary(self, prim, alpha, beta):
        return np.stack([1.0 - alpha - beta, alpha, beta], -1)

    def point(self, prim, alpha, beta):
        """S of base triangle(s) `prim` at (alpha, beta); everything broadcasts."""
        w = self.bary(prim, alpha, beta)
        P = np.einsum("...k,...kc->...c", w, self.p[prim])
        N = np.einsum("...k,...kc->...c", w, self.n[prim])
        tc = np.einsum("...k,...kc->...c", w, self.tc[prim])
        return P + (self.base + self.scale * self.height(tc))[..., None] * N

    def patch(self, prim, alpha, beta, piece=None):
        """S, dS/dalpha, dS/dbeta on the affine height piece `piece` (default: the one (alpha, beta) lies in)."""
        w = self.bary(prim, alpha, beta)
        p, n, t = self.p[prim], self.n[prim], self.tc[prim]
        P, N, tc = (np.einsum("...k,...kc->...c", w, a) for a in (p, n, t))
        if piece is None:
            piece = self.piece(tc)[:5]
        h0, gu, gv, u0, v0 = piece
        s = tc * self.res
        H = self.base + self.scale * (h0 + gu * (s[..., 0] - u0) + gv * (s[..., 1] - v0))
        dtA, dtB = (t[..., 1, :] - t[..., 0, :]) * self.res, (t[..., 2, :] - t[..., 0, :]) * self.res
        HA, HB = self.scale * (gu * dtA[..., 0] + gv * dtA[..., 1]), self.scale * (gu * dtB[..., 0] + gv * dtB[..., 1])
        SA = (p[..., 1, :] - p[..., 0, :]) + HA[..., None] * N + H[..., None] * (n[..., 1, :] - n[..., 0, :])
        SB = (p[..., 2, :] - p[..., 0, :]) + HB[..., None] * N + H[..., None] * (n[..., 2, :] - n[..., 0, :])
        return P + H[..., None] * N, SA, SB, N

    def normal(self, prim, alpha, beta):
        """The unit normal of the patch, on the side of growing height."""
        _, SA, SB, N = self.patch(prim, alpha, beta)
        c = np.cross(SA, SB)
        c *= np.sign((c * N).sum(-1))[..., None]
        return c / np.linalg.norm(c, axis=-1, keepdims=True)

    # ---- facets
    def facets(self, ti, k):
        """Flat facets of base triangle `ti`: texture coordinates [F, 3, 2] and points on S [F, 3, 3] of the k x k sub-triangles of
        every half texel that overlaps the footprint."""
        tc = self.tc[ti]
        n = self.res
        x0, y0, x1, y1 = T.texel_range(tc, n)
        xs, ys = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1))
        xs, ys = xs.ravel(), ys.ravel()
        keep = T.overlap_sat(tc, (xs + 0.5) / n, (ys + 0.5) / n, 0.5 / n)
        xs, ys = xs[keep].astype(np.float64), ys[keep].astype(np.float64)
        out = []
        for a in range(k):
            for b in range(k - a):
                # sub-triangles of the unit half texel {(i, j): 0 <= j <= i <= 1} in its own barycentric grid
                cells = [((a, b), (a + 1, b), (a, b + 1))]
                if a + b + 1 < k:
                    cells.append(((a + 1, b), (a + 1, b + 1), (a, b + 1)))
                for cell in cells:
                    for upper in (True, False):
                        pts = []
                        for (i, j) in cell:
                            # grid (i, j) / k: i steps along the first edge from TL, j along the second
                            e1, e2 = ((1.0, 0.0), (0.0, 1.0)) if upper else ((0.0, 1.0), (1.0, 0.0))      # TL->TR, TR->BR | TL->BL, BL->BR
                            fu = (i + j) / k * e1[0] + j / k * e2[0]
                            fv = (i + j) / k * e1[1] + j / k * e2[1]
                            pts.append(np.stack([(xs + fu) / n, (ys + fv) / n], -1))
                        out.append(np.stack(pts, 1))
        ft = np.concatenate(out)                                            # [F, 3, 2]
        # heights from the half texel's own affine piece (taken at the facet's centroid, so that shared corners get their own side)
        cen = ft.mean(1)
        h0, gu, gv, u0, v0 = self.piece(cen)[:5]
        s = ft * n
        h = h0[:, None] + gu[:, None] * (s[..., 0] - u0[:, None]) + gv[:, None] * (s[..., 1] - v0[:, None])
        toBc = np.linalg.inv(np.stack([tc[:, 0], tc[:, 1], np.ones(3)]))
        w = np.concatenate([ft, np.ones(ft.shape[:-1] + (1,))], -1) @ toBc.T
        P, N = w @ self.p[ti], w @ self.n[ti]
        tile = np.stack([np.floor(cen[:, 0] * n).astype(np.int64) // TILE, np.floor(cen[:, 1] * n).astype(np.int64) // TILE], 1)
        return ft, P + (self.base + self.scale * h)[..., None] * N, tile

    def chunks(self, k):
        """The facets in groups that a sphere encloses tightly: per base triangle, per TILE x TILE block of texels.  [(ti, ft, fp, centre, radius)]"""
        out = []
        for ti in range(len(self.p)):
            if T._cross2(self.tc[ti, 1] - self.tc[ti, 0], self.tc[ti, 2] - self.tc[ti, 0]) == 0:
                continue
            ft, fp, tile = self.facets(ti, k)
            if not len(ft):
                continue
            _, inv = np.unique(tile, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            for g in range(inv.max() + 1):
                sel = inv == g
                pts = fp[sel].reshape(-1, 3)
                centre = 0.5 * (pts.min(0) + pts.max(0))
                # the exact patches bulge from their flat facets by a second-order term; a tenth of the group's size covers it many times
                out.append((ti, ft[sel], fp[sel], centre, np.linalg.norm(pts - centre, axis=1).max() * 1.1 + 1e-9 * self.extent))
        return out

    # ---- rays
    def trace(self, org, d, tmin, tmax, k=2, eps=1e-3, flags=True, exact=False):
        """Closest hit per ray: dict t (inf: miss), prim, alpha, beta, and with `flags` the edge rule's `flagged`."""
        org, d = org.astype(np.float64), d.astype(np.float64)
        tmin, tmax = np.asarray(tmin, np.float64), np.asarray(tmax, np.float64)
        R = len(org)
        best = {"t": np.full(R, np.inf), "prim": np.full(R, -1), "alpha": np.zeros(R), "beta": np.zeros(R)}
        flagged = np.zeros(R, bool)
        grazing = np.zeros(R, bool)
        retry = np.zeros(R, bool)            # a flat facet was hit, but Newton from there found no root on that base triangle
        ok = np.isfinite(org).all(1) & np.isfinite(d).all(1) & ((d * d).sum(1) > 0)
        dn = np.where(ok[:, None], d, 1.0)
        dn = dn / np.linalg.norm(dn, axis=1, keepdims=True)

        def near_rays(centre, radius):
            oc = centre - org
            return np.nonzero(ok & (np.linalg.norm(oc - (oc * dn).sum(1)[:, None] * dn, axis=1) <= radius))[0]

        for ti, ft, fp, centre, radius in (() if exact else self.chunks(k)):
            idx = near_rays(centre, radius)
            if not len(idx):
                continue
            clip = (ft[:, 0], ft[:, 1], ft[:, 2], np.broadcast_to(self.tc[ti], (len(ft), 3, 2)), np.zeros(len(ft), np.int64))
            t, fk, _, _ = T.brute64(fp[:, 0], fp[:, 1], fp[:, 2], org[idx], d[idx], tmin[idx], tmax[idx], clip=clip, eps=eps)
            hit = np.isfinite(t)
            if not hit.any():
                continue
            ridx, fk = idx[hit], fk[hit]
            a, b, tt, good = self._polish(ti, ft[fk], fp[fk], org[ridx], d[ridx], t[hit])
            retry[ridx[~good]] = True
            grazing[ridx[~good]] = True
            better = good & (tt > tmin[ridx]) & (tt < tmax[ridx]) & ((tt < best["t"][ridx]) | ((tt == best["t"][ridx]) & (ti < best["prim"][ridx])))
            r = ridx[better]
            best["t"][r], best["prim"][r], best["alpha"][r], best["beta"][r] = tt[better], ti, a[better], b[better]
        # ... and so may a ray that met no flat facet at all.  exact: every ray goes through the second stage (a mesh whose patches
        # are strongly curved, where a flat facet can hide a nearer patch)
        retry |= ok & (~np.isfinite(best["t"]) | exact)
        if retry.any():
            # Such a ray meets the surface on a neighbouring base triangle, or grazes the patch's bulge over its flat facet.  Newton from
            # the centre of EVERY half texel near the ray, on every base triangle: exact, and affordable for these few rays.
            found = np.zeros(R, bool)
            seeds = np.array([[1 / 3, 1 / 3], [0.6, 0.2], [0.2, 0.6], [0.2, 0.2]])
            batch, pairs = [], 0

            def flush():
                ti, ft, fp, ri, sd = (np.concatenate(x) for x in zip(*batch))
                t0 = ((fp.mean(1) - org[ri]) * d[ri]).sum(1) / (d[ri] * d[ri]).sum(1)
                a, b, tt, good = self._polish(ti, ft, fp, org[ri], d[ri], t0, reseed=False, seed=sd)
                good &= (tt > tmin[ri]) & (tt < tmax[ri])
                ri, ti, a, b, tt = ri[good], ti[good], a[good], b[good], tt[good]
                order = np.lexsort((ti, tt, ri))
                ri, ti, a, b, tt = ri[order], ti[order], a[order], b[order], tt[order]
                first = np.ones(len(ri), bool)
                first[1:] = ri[1:] != ri[:-1]
                r, ti, a, b, tt = ri[first], ti[first], a[first], b[first], tt[first]
                found[r] = True
                better = (tt < best["t"][r]) | ((tt == best["t"][r]) & (ti < best["prim"][r]))
                r = r[better]
                best["t"][r], best["prim"][r], best["alpha"][r], best["beta"][r] = tt[better], ti[better], a[better], b[better]

            for ti, ft, fp, centre, radius in self.chunks(1):
                oc = centre - org
                idx = np.nonzero(retry & (np.linalg.norm(oc - (oc * dn).sum(1)[:, None] * dn, axis=1) <= radius))[0]
                if not len(idx):
                    continue
                # four starts per half texel (its centre and a point toward each corner): a patch is quadratic, a ray can meet it twice
                fi = np.tile(np.repeat(np.arange(len(ft)), 4), len(idx))
                batch.append((np.full(len(fi), ti), ft[fi], fp[fi], np.repeat(idx, 4 * len(ft)), np.tile(seeds, (len(idx) * len(ft), 1))))
                pairs += len(fi)
                if pairs > 400000:
                    flush()
                    batch, pairs = [], 0
            if batch:
                flush()
            # no root anywhere near the flat facet that was hit: the ray grazes; it counts as an edge ray (tests' docstrings)
            flagged |= grazing & ~found
        if flags:
            # The edge rule on the half texels themselves (k = 1: the micro-triangles the query intersects), up to the closest hit:
            # its own barycentrics, and anything nearer that the ray passes within eps outside of.
            upto = np.where(np.isfinite(best["t"]), best["t"] * (1 + 1e-9) + 1e-12 * self.extent, tmax)
            for ti, ft, fp, centre, radius in (self.chunks(1) if k != 1 else self.chunks(k)):
                idx = near_rays(centre, radius * 1.05)
                if not len(idx):
                    continue
                clip = (ft[:, 0], ft[:, 1], ft[:, 2], np.broadcast_to(self.tc[ti], (len(ft), 3, 2)), np.zeros(len(ft), np.int64))
                _, _, edge, near = T.brute64(fp[:, 0], fp[:, 1], fp[:, 2], org[idx], d[idx], tmin[idx], upto[idx], clip=clip, eps=eps)
                flagged[idx] |= edge | near
            h = np.isfinite(best["t"])
            a, b, pr = best["alpha"][h], best["beta"][h], best["prim"][h]
            w = np.stack([1 - a - b, a, b], -1)
            tc = np.einsum("rk,rkc->rc", w, self.tc[pr])
            fu, fv = self.piece(tc)[6]
            micro = np.minimum(np.minimum(np.abs(fu - fv), np.minimum(fu, fv)), np.minimum(1 - fu, 1 - fv))
            fl = flagged[h]
            fl |= (w.min(-1) < eps) | (micro < eps)
            flagged[h] = fl
        best["flagged"] = flagged
        return best

    def _polish(self, ti, ft, fp, org, d, t0, reseed=True, seed=None):
        """Newton in (alpha, beta, t) on the exact patch of the half texel each candidate facet belongs to, from the facet hit."""
        ti = np.broadcast_to(np.asarray(ti), (len(ft),))
        tcs = self.tc[ti]                                                  # [R, 3, 2]
        toBc = np.linalg.inv(np.stack([tcs[:, :, 0], tcs[:, :, 1], np.ones((len(ft), 3))], 1))
        hp = org + t0[:, None] * d
        # barycentrics of the facet hit -> texture coordinate -> (alpha, beta)
        e1, e2 = fp[:, 1] - fp[:, 0], fp[:, 2] - fp[:, 0]
        rel = hp - fp[:, 0]
        g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        r1, r2 = (rel * e1).sum(1), (rel * e2).sum(1)
        det = g11 * g22 - g12 * g12
        u, v = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
        if seed is not None:               # from given points of the half texel, not from a facet hit
            u, v = seed[:, 0], seed[:, 1]
        tc = ft[:, 0] + u[:, None] * (ft[:, 1] - ft[:, 0]) + v[:, None] * (ft[:, 2] - ft[:, 0])
        w = np.einsum("rk,rjk->rj", np.concatenate([tc, np.ones((len(tc), 1))], 1), toBc)
        a, b, t = w[:, 1].copy(), w[:, 2].copy(), t0.copy()
        # Newton on the affine height piece the candidate facet belongs to; a root that lands in another half texel is not a root of the
        # surface: the iteration is re-seeded on the piece it landed in, until it lands where it was solved (at most 4 times)
        full = self.piece(ft.mean(1))
        piece, ident = [np.array(x, np.float64) for x in full[:5]], np.stack([full[5][0], full[5][1], full[5][2].astype(np.int64)], 1)
        good = np.zeros(len(a), bool)
        live = np.ones(len(a), bool)
        for _ in range(4 if reseed else 1):
            for _ in range(12):
                S, SA, SB, _ = self.patch(ti, a, b, piece)
                F = S - org - t[:, None] * d
                J = np.stack([SA, SB, -d], -1)
                with np.errstate(all="ignore"):
                    try:
                        step = np.linalg.solve(J, F[..., None])[..., 0]
                    except np.linalg.LinAlgError:
                        step = np.einsum("rij,rj->ri", np.linalg.pinv(np.nan_to_num(J)), F)
                step[~live] = 0.0
                a, b, t = a - step[:, 0], b - step[:, 1], t - step[:, 2]
            S = self.patch(ti, a, b, piece)[0]
            res = np.linalg.norm(S - org - t[:, None] * d, axis=1)
            in_base = np.minimum(np.minimum(a, b), 1 - a - b) >= -1e-9
            fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(t)
            a, b, t = np.where(fin, a, 0.3), np.where(fin, b, 0.3), np.where(fin, t, 0.0)
            tcn = np.einsum("rk,rkc->rc", np.stack([1 - a - b, a, b], -1), tcs)
            s = tcn * self.res
            fu, fv = s[:, 0] - piece[3], s[:, 1] - piece[4]
            upper = ident[:, 2] == 1
            inside = np.where(upper, (fv >= -1e-9) & (fu <= 1 + 1e-9) & (fu - fv >= -1e-9), (fu >= -1e-9) & (fv <= 1 + 1e-9) & (fv - fu >= -1e-9))
            done = live & fin & (res < 1e-12 * self.extent) & inside & in_base
            good |= done
            live &= ~done & fin & in_base & (res < 1e-12 * self.extent)      # converged, inside the base triangle, in another half texel
            if not live.any():
                break
            landed = self.piece(tcn)
            for i in range(5):
                piece[i] = np.where(live, landed[i], piece[i])
            ident = np.where(live[:, None], np.stack([landed[5][0], landed[5][1], landed[5][2].astype(np.int64)], 1), ident)
        return a, b, t, good
