"""TEST INFRASTRUCTURE: synthetic input sequences for the SVGF denoiser (gfx_denoise), numpy only.  One frame holds, on an image of any
size from 1 x 1 up, what a rendered frame rarely or never does: guide edges that cross the 16-pixel workgroup tiles, albedo on both
sides of the demodulation threshold, flow vectors exactly on the bounds of the reprojection, a footprint with only its right-hand (or
lower) taps on screen, non-finite flow.  tests/test_denoise_cases_cpu.py shows on the restatement that the sequences reach the history
classes the comparison of tests/test_gpu_denoise_edges.py relies on; the invariants at the end are functions of (inputs, output,
history) alone and serve both files.  Step numbers cite the specification in the header of gfxexp_amd/csrc/denoise/denoise.hip."""
import numpy as np

BOX3X3, GAUSS3X3, GAUSS5X5 = 0, 1, 2
RADIUS = {BOX3X3: 1, GAUSS3X3: 1, GAUSS5X5: 2}
TAPS = {BOX3X3: 8, GAUSS3X3: 8, GAUSS5X5: 24}

# narrower than a tile, narrower than a halo, one pixel wide or high (W / 2 == 0 turns the depth gradient), one under / on / one over
# the 16-pixel tile, and two sizes with several partial workgroups
SIZES = [(1, 1), (1, 37), (17, 1), (2, 2), (15, 15), (16, 16), (17, 17), (37, 23), (49, 33)]
FRAMES = 6

# stage i runs at step 2^i: k_dn_atrous<K, R, LAST> with R = KR (step 1), 2 KR (step 2), 0 (wider), LAST on the last stage, so per table
#   numStages 1: <K, KR, true>
#   numStages 2: <K, KR, false> <K, 2KR, true>
#   numStages 3: <K, KR, false> <K, 2KR, false> <K, 0, true>
#   numStages 4: <K, KR, false> <K, 2KR, false> <K, 0, false> <K, 0, true>
# (KR = 1 for Box3x3 and Gauss3x3, 2 for Gauss5x5): the first twelve settings launch all 18 instantiations
SETTINGS = [dict(kernel=k, numStages=s) for k in (BOX3X3, GAUSS3X3, GAUSS5X5) for s in (1, 2, 3, 4)] + [
    dict(numStages=0), dict(numStages=5), dict(feedbackStage=0), dict(minAlpha=0.0), dict(sigmaN=1.0), dict(sigmaN=1024.0),
    dict(sigmaZ=0.01)]

_F = np.float32
# two normals 0.95 apart (above the 0.85 acceptance of step 3) and one orthogonal to both
NORMALS = np.array([(0.0, 0.0, 1.0), (np.sqrt(1.0 - 0.95 * 0.95), 0.0, 0.95), (0.0, 1.0, 0.0)], np.float32)
ALBEDO_EDGE = np.array([_F(1e-3), _F(0.0), np.nextafter(_F(1e-3), _F(1.0))], np.float32)    # a > 1e-3 fails, fails, holds


def reprojected(x, f):
    """fx of step 3 for pixel coordinate x and flow component f, in float32 and in the specification's order."""
    return ((_F(x) + _F(0.5)) - _F(f)) - _F(0.5)


def _flow_inside(x, bound):
    """The flow component next to x - bound (where fx is exactly `bound`, -1 or the image size, and gives no tap) that puts fx
    strictly inside.  fx = nextafter(-1, 0) comes out only at x = 0: for x >= 1 the floats around x + 1 are 2^-23 or more apart,
    so the fx nearest to -1 is -1 + 2^-23."""
    assert reprojected(x, x - bound) == _F(bound)
    inside = (lambda v: v > _F(-1.0)) if bound < 0 else (lambda v: v < _F(bound))
    for k in range(-24, 0):                                # the smallest power of two that survives the roundings of fx
        f = _F(x - bound) + (_F(-2.0 ** k) if bound < 0 else _F(2.0 ** k))
        if inside(reprojected(x, f)):
            return f
    raise AssertionError("no flow puts pixel %d just inside %d" % (x, bound))


def _border_flow(n):
    """Flow component along an axis of n pixels for the border cases, as (pixel, [candidates]): pixel 0 sits exactly on -1 (no tap)
    or on nextafter(-1, 0) (x0 = -1: only the taps at 0 are on screen), pixel 1 as close above -1 as it gets, pixel n - 1 just under
    n (x0 = n - 1: only the taps at n - 1 are on screen).  Where an axis is too short to keep them apart they share a pixel."""
    cases = {0: [_F(1.0), _flow_inside(0, -1)]}
    if n >= 2:
        cases.setdefault(1, []).append(_flow_inside(1, -1))
    cases.setdefault(n - 1, []).append(_flow_inside(n - 1, n))
    return sorted(cases.items())


def _block(mask, x0, y0, bw, bh):
    mask[max(y0, 0):y0 + bh, max(x0, 0):x0 + bw] = True


def layout(w, h):
    """The static geometry of a w x h sequence, (h, w) arrays: the normal band 0..2 (diagonal edges), the block of raised depth, the
    geometric background and the emissive block.  Every block is left out where the image cannot hold it."""
    yy, xx = np.mgrid[0:h, 0:w]
    d, t = xx + yy, w + h
    band = (3 * d >= t).astype(np.int64) + (3 * d >= 2 * t)
    raised = np.zeros((h, w), bool)
    if w >= 3 and h >= 3:
        _block(raised, w // 3, h // 3, max(1, w // 4), max(1, h // 3))
    bw, bh = max(1, w // 8), max(1, h // 8)
    bg = np.zeros((h, w), bool)
    if w >= 4 and h >= 4:
        _block(bg, w - 1 - bw, 1, bw, bh)                  # upper right, one pixel off the border
    elif w * h >= 4:
        bg[h // 4, w - 1] = True
    emissive = np.zeros((h, w), bool)
    if w >= 4 and h >= 4:
        _block(emissive, 1, h - 1 - bh, bw, bh)            # lower left
    elif w * h >= 4:
        emissive[h - 1 - h // 4, w // 4] = True
    return band, raised, bg, emissive


def make_frame(rng, w, h, f):
    """Frame f of a sequence: (beauty float32[n, 4], albedo [n, 4], normal [n, 4], flow [n, 2], depth [n], emissive int32[n]), n = w h
    row-major.  The geometry is the same in every frame; beauty, albedo and flow are drawn anew, and a block of far flow moves."""
    band, raised, bg, em = layout(w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    normal = np.ones((h, w, 4), np.float32)
    normal[..., :3] = NORMALS[band]
    normal[bg, :3] = 0.0                                   # background without a depth guide
    depth = (_F(5.0) + _F(0.05) * xx.astype(np.float32) + _F(0.02) * yy.astype(np.float32)).astype(np.float32)
    depth[raised] += _F(3.0)                               # 3 > 0.1 z: a tap across the block's edge fails the depth test
    depth[bg] = np.inf                                     # background with one
    emissive = em.astype(np.int32) * (1 + (xx + yy) % 3).astype(np.int32)     # any non-zero value counts

    albedo = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    albedo[..., 3] = 1.0
    edge = rng.random((h, w)) < 0.05
    turn = rng.integers(0, 3, (h, w))
    for k in range(3):
        albedo[..., k] = np.where(edge, ALBEDO_EDGE[(turn + k) % 3], albedo[..., k])
    beauty = rng.uniform(0.0, 3.0, (h, w, 4)).astype(np.float32)

    flow = rng.uniform(-2.5, 2.5, (h, w, 2)).astype(np.float32)
    flow[rng.random((h, w)) < 0.4] = 0.0                   # history survives in place and lengths grow
    for x, cand in _border_flow(w):
        for y in range(h):
            flow[y, x, 0] = cand[(y + f) % len(cand)]
    for y, cand in _border_flow(h):
        for x in range(w):
            flow[y, x, 1] = cand[(x + f) % len(cand)]
    if w >= 8 and h >= 4:                                  # far off screen: restarts, at another place in every frame
        far = np.zeros((h, w), bool)
        fw, fh = max(2, w // 7), max(2, h // 3)
        _block(far, 2 + (f * fw) % (w - 3 - fw), h // 2 - 1, fw, fh)
        flow[far] = (40.0, -25.0)
    if w * h >= 9:
        flow[(2 * h) // 3, w // 2] = (np.nan, 0.0)
        flow[h // 3, (2 * w) // 3] = (np.inf, 0.0)
    n = w * h
    return (beauty.reshape(n, 4), albedo.reshape(n, 4), normal.reshape(n, 4), flow.reshape(n, 2), depth.reshape(n), emissive.reshape(n))


def sequence(w, h, frames=FRAMES, seed=None):
    rng = np.random.default_rng(1000 * w + h if seed is None else seed)
    return [make_frame(rng, w, h, f) for f in range(frames)]


def _constant(w, h, normal):
    n = w * h
    nrm = np.ones((n, 4), np.float32); nrm[:, :3] = normal
    alb = np.full((n, 4), 0.5, np.float32)
    return nrm, alb, np.zeros((n, 2), np.float32), np.full(n, 6.0, np.float32), np.zeros(n, np.int32)


CAP_CALLS = 258


def cap_sequence(w=9, h=7, calls=CAP_CALLS):
    """Constant guides, zero flow, random beauty: every length counts 1, 2, ... and stops at 255."""
    rng = np.random.default_rng(255)
    nrm, alb, flow, depth, em = _constant(w, h, NORMALS[0])
    return [(rng.uniform(0.0, 3.0, (w * h, 4)).astype(np.float32), alb, nrm, flow, depth, em) for _ in range(calls)]


HALF_FLOW_FROM = 5


def half_sequence(w=9, h=7, frames=8):
    """Lengths an odd number apart side by side, then a flow of half a pixel.  The right columns hold NORMALS[2] throughout; the left
    four start on NORMALS[0] and change to NORMALS[2] at frame 3 for good, which restarts them: lengths 1 | 4 after frame 3, 2 | 5
    after frame 4.  From frame HALF_FLOW_FROM the flow is (0.5, 0): x0 = x - 1, both taps of a row weigh exactly 1/2, and column 4
    blends 2 and 5: nf / sw = 3.5."""
    rng = np.random.default_rng(52)
    right, alb, flow0, depth, em = _constant(w, h, NORMALS[2])
    left = right.copy()
    left.reshape(h, w, 4)[:, :4, :3] = NORMALS[0]
    flow1 = flow0.copy(); flow1[:, 0] = 0.5
    return [(rng.uniform(0.0, 3.0, (w * h, 4)).astype(np.float32), alb, left if f < 3 else right, flow1 if f >= HALF_FLOW_FROM else flow0,
             depth, em) for f in range(frames)]


# ---------------------------------------------------------------- the lengths of step 3, recomputed from the inputs
def background(frame, with_depth, with_emissive):
    """bg(p) of the specification, bool[n]."""
    _, _, normal, _, depth, emissive = frame
    bg = depth == np.inf if with_depth else np.all(normal[:, :3] == 0.0, axis=1)
    return bg | (emissive != 0) if with_emissive else bg


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]       # float32 scalars, left to right


def new_length(sw, nf):
    """n of step 3 from reproject()'s sums: min(roundf(nf / sw) + 1, 255), 1 without an accepted tap (v - floor(v) is exact)."""
    v = nf / np.where(sw > 0, sw, _F(1.0))
    k = np.floor(v)
    r = k + (v - k >= _F(0.5))
    return np.where(sw > 0, np.minimum(r + 1, 255), 1).astype(np.uint32)


def reproject(w, h, frame, prev_frame, prev_length, with_depth, with_emissive):
    """Step 3's tap selection for one call that is not a first frame, from the inputs and the lengths the previous call left alone.
    Returns per pixel (sw, nf, partly) as float32, float32, bool: the sums of the accepted taps' weights and of weight x length, and
    whether a tap was accepted while another tap of the footprint was off screen."""
    _, _, normal, flow, depth, _ = frame
    pnormal, pdepth = prev_frame[2], prev_frame[4]
    bg = background(frame, with_depth, with_emissive)
    sw, nf, partly = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32), np.zeros(w * h, bool)
    one = _F(1.0)
    for p in range(w * h):
        if bg[p]:
            continue
        x, y = p % w, p // w
        fx, fy = reprojected(x, flow[p, 0]), reprojected(y, flow[p, 1])
        if not (fx > _F(-1.0) and fx < _F(w) and fy > _F(-1.0) and fy < _F(h)):
            continue
        bx, by = np.floor(fx), np.floor(fy)
        s, t = fx - bx, fy - by
        x0, y0 = int(bx), int(by)
        weights = ((one - s) * (one - t), s * (one - t), (one - s) * t, s * t)
        off = hit = False
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            if qx < 0 or qx >= w or qy < 0 or qy >= h:
                off = True
                continue
            q = qy * w + qx
            if prev_length[q] == 0 or not _dot(pnormal[q], normal[p]) > _F(0.85):
                continue
            if with_depth and not abs(pdepth[q] - depth[p]) <= _F(0.1) * depth[p]:
                continue
            hit = True
            sw[p] = sw[p] + weights[k]
            nf[p] = nf[p] + weights[k] * _F(prev_length[q])
        partly[p] = off and hit
    return sw, nf, partly


# ---------------------------------------------------------------- invariants: functions of (inputs, output, history), no restatement
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_background(frame, out, hist, with_depth, with_emissive):
    """(a) step 1: a background or emissive pixel outputs its beauty bit for bit, and its history is lighting 0, moments 0, length 0."""
    bg = background(frame, with_depth, with_emissive)
    n = len(bg)
    assert np.array_equal(_bits(out).reshape(n, 4)[bg], _bits(frame[0])[bg])
    assert not _bits(hist["lighting"]).reshape(n, 4)[bg].any() and not _bits(hist["moments"]).reshape(n, 2)[bg].any()
    assert not np.asarray(hist["length"]).reshape(n)[bg].any()
    return int(bg.sum())


def check_zero_stages_first_frame(frame, out, with_depth, with_emissive):
    """(b) steps 2 and 6 with nothing between (numStages = 0, a first frame): out.k = a.k > 1e-3 ? (c.k / a.k) * a.k : c.k in float32,
    out.w = beauty.w, on every pixel that is not background."""
    beauty, albedo = frame[0], frame[1]
    fg = ~background(frame, with_depth, with_emissive)
    c, a = beauty[:, :3], albedo[:, :3]
    big = a > _F(1e-3)
    want = np.where(big, (c / np.where(big, a, _F(1.0))) * a, c).astype(np.float32)
    out =np.asarray(out).reshape(-1, 4)
    assert np.array_equal(_bits(out[:, :3])[fg], _bits(want)[fg])
    assert np.array_equal(_bits(out[:, 3])[fg], _bits(beauty[:, 3])[fg])
    return int(fg.sum())


def check_one_stage_within_footprint(w, h, kernel, frame, hist, with_depth, with_emissive):
    """(c) numStages = 1, feedbackStage = 1, a first frame, albedo 0 everywhere (L of step 2 is the beauty itself): the history
    lighting is stage 0's A.k / sw, a mean of L over the on-screen, non-background taps of the table with weights >= 0 (the centre's
    is > 0), so per channel it lies within the minimum and maximum of the beauty over that footprint, up to rounding."""
    beauty, albedo = frame[0], frame[1]
    assert not albedo[:, :3].any() and beauty.min() >= 0.0
    bg = background(frame, with_depth, with_emissive).reshape(h, w)
    L = beauty[:, :3].reshape(h, w, 3).astype(np.float64)
    got = np.asarray(hist["lighting"], np.float32).reshape(h, w, 4).astype(np.float64)
    # Rounding: A.k is a sum of T + 1 products, each rounded once and then carried through at most T additions: every term w_i L_i
    # picks up at most T + 1 factors (1 + d), |d| <= u = 2^-24.  sw is T additions of the weights: at most T factors per term.  One
    # division: one more.  With all terms >= 0 the quotient is min..max of L times at most 2T + 2 such factors, and
    # (1 + u)^(2T + 2) <= 1 + (2T + 4) u = 1 + (T + 2) 2^-23 for the T of these tables (the second-order part, (2T + 2)^2 u^2 / 2 <
    # 2e-11, is far under the 2u to spare).  A textbook bound, not a measured one.
    slack = (TAPS[kernel] + 2) * 2.0 ** -23
    r = RADIUS[kernel]
    checked = 0
    for y in range(h):
        for x in range(w):
            if bg[y, x]:
                continue
            ys, xs = slice(max(y - r, 0), y + r + 1), slice(max(x - r, 0), x + r + 1)
            taps = L[ys, xs][~bg[ys, xs]]
            lo, hi = taps.min(axis=0) * (1.0 - slack), taps.max(axis=0) * (1.0 + slack)
            assert np.all(got[y, x, :3] >= lo) and np.all(got[y, x, :3] <= hi), (x, y, got[y, x, :3], lo, hi)
            checked += 1
    return checked
