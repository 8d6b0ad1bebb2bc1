"""The contract of stereo rectification, in plain numpy (the style of tools/undistort_model.py, which it imports): what
ssx_stereo_rectify computes on the host for a raw rig, and what ssx_undistort_lens / ssx_undistort_plan_add_lens (csrc/undistort.hip:
ud_map) compute per pixel for the two lens models.  f64 throughout, every operation rounded on its own in the order written; dot and
cross products are written out element by element (no BLAS, which may fuse or reorder).  DESIGN.md 6n.

rectify(rig) -- the common rectified camera.  Only + - * / sqrt, each correctly rounded by IEEE, so a C++ restatement compiled without
contraction gives the same bits (this rules out Bouguet's half-rotation of cv::stereoRectify, which needs acos / sin / cos).
With X_right = R X_left + t, R row-major, in the left camera's frame:

    c[i]  = ((-R[0][i])*t[0] + (-R[1][i])*t[1]) + (-R[2][i])*t[2]          the right camera's centre, -R^T t
    b     = sqrt((c[0]*c[0] + c[1]*c[1]) + c[2]*c[2]);   e1[i] = c[i] / b
    zm    = (0 + R[2][0], 0 + R[2][1], 1 + R[2][2])                         the sum of the two optical axes
    d     = (zm[0]*e1[0] + zm[1]*e1[1]) + zm[2]*e1[2];   e3'[i] = zm[i] - d*e1[i]
    n2    = (e3'[0]*e3'[0] + e3'[1]*e3'[1]) + e3'[2]*e3'[2];   n = sqrt(n2);   e3[i] = e3'[i] / n
    e2    = (e3[1]*e1[2] - e3[2]*e1[1],  e3[2]*e1[0] - e3[0]*e1[2],  e3[0]*e1[1] - e3[1]*e1[0])          e3 x e1
    R_l   = rows e1, e2, e3;   R_r[i][j] = (R_l[i][0]*R[j][0] + R_l[i][1]*R[j][1]) + R_l[i][2]*R[j][2]    R_l R^T
    f     = ((fx_l + fy_l) + (fx_r + fy_r)) / 4;  cx = (cx_l + cx_r) / 2;  cy = (cy_l + cy_r) / 2        unless the caller gives them
    newK  = (f, f, cx, cy)
    g = 1/f;  mx = -cx/f;  my = -cy/f                                       newK^-1 = [g 0 mx; 0 g my; 0 0 1]
    iR[3i+0] = S[0][i]*g;  iR[3i+1] = S[1][i]*g;  iR[3i+2] = (S[0][i]*mx + S[1][i]*my) + S[2][i]         S^T newK^-1, S = R_l or R_r

(in iR[3i+2] the left-most product is taken first).  A point X of the left frame has the rectified coordinates R_l X in the left and
R_l X - (b, 0, 0) in the right camera: equal rows, equal depths, a disparity of f*b/z.

Refusals (ValueError; REASONS holds the texts, ssx_stereo_rectify writes the same ones): an unknown lens model, a non-finite input,
b == 0, max|R R^T - I| > 1e-6 (a validity condition on the input), e1[0] <= 0 (the right camera is not to the right), n2 < 1e-12 (the
optical axes lie along the baseline).

lens_map(rows, cols, model, K, coeffs, iR) -- (iu, iv), the quantised source positions.  RADTAN is undistort_model.undistort_map.  KB4
(Kannala-Brandt "equidistant", coeffs = k1 k2 k3 k4) is the same chain up to x, y, then

    r2 = x*x + y*y;  r = sqrt(r2);  th = atan_c(r);  t2 = th*th
    thd = th * (1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))))
    s = 1 if r == 0 else thd / r
    u = fx*(x*s) + cx;  v = fy*(y*s) + cy
    where not (W > 0): u = v = -inf            behind the camera, or NaN: every tap is outside, so the pixel is 0
    iu = q(u*32), iv = q(v*32)                 q and everything behind it (remap, pack_map) are undistort_model's

atan is no IEEE-rounded operation, so atan_c(r), r >= 0, is stated here in f64 operations: the classical argument reduction at 7/16,
11/16, 19/16 and 39/16 with high / low constants, and an 11-term odd polynomial in two Horner halves.  At and above 2^66 it is
pi/2; NaN gives NaN.

Deviations from OpenCV: cv::stereoRectify rotates both cameras by half of R (acos / sin / cos) and then aligns the baseline, this
construction takes the baseline and the mean optical axis directly; there is no alpha scaling and no valid-ROI, the principal point
is the mean or the caller's.  cv::fisheye::initUndistortRectifyMap evaluates theta with the library's atan and rows incrementally,
and leaves pixels with W <= 0 undefined; here they are 0.

unrectify_image and rot are NOT part of the contract: test inputs only."""
import numpy as np

from tools import undistort_model as um

RADTAN, KB4 = 0, 1
MODEL_NAMES = {"radtan": RADTAN, "kb4": KB4}

REASONS = {
    "model": "unknown lens model",
    "finite": "a non-finite input",
    "baseline": "the baseline is zero",
    "rotation": "R is not a rotation: max|R R^T - I| > 1e-6",
    "side": "the right camera is not to the right of the left one (e1[0] <= 0)",
    "axes": "the optical axes lie along the baseline (|e3'|^2 < 1e-12)",
}

_F = np.float64
ATAN_HI = (_F(4.63647609000806093515e-01), _F(7.85398163397448278999e-01), _F(9.82793723247329054082e-01), _F(1.57079632679489655800e+00))
ATAN_LO = (_F(2.26987774529616870924e-17), _F(3.06161699786838301793e-17), _F(1.39033110312309984516e-17), _F(6.12323399573676603587e-17))
ATAN_T = tuple(_F(v) for v in (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                               9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                               4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02))
ATAN_BIG = _F(2.0) ** 66


def atan_c(r):
    """atan of r >= 0 (any shape), in f64 operations in this order:

        r < 7/16:   id = -1, t = r
        r < 11/16:  id = 0,  t = (2*r - 1) / (2 + r)
        r < 19/16:  id = 1,  t = (r - 1) / (r + 1)
        r < 39/16:  id = 2,  t = (r - 1.5) / (1 + 1.5*r)
        else:       id = 3,  t = -1 / r
        z = t*t;  w = z*z
        s1 = z*(T0 + w*(T2 + w*(T4 + w*(T6 + w*(T8 + w*T10)))))
        s2 = w*(T1 + w*(T3 + w*(T5 + w*(T7 + w*T9))))
        id = -1: t - t*(s1 + s2);   else: HI[id] - ((t*(s1 + s2) - LO[id]) - t)
        r >= 2^66: HI[3];   r is NaN: NaN"""
    r = np.asarray(r, dtype=np.float64)
    one, two, h = _F(1.0), _F(2.0), _F(1.5)
    T = ATAN_T
    with np.errstate(all="ignore"):
        c0, c1, c2, c3 = r < _F(0.4375), r < _F(0.6875), r < _F(1.1875), r < _F(2.4375)
        num = np.where(c1, two * r - one, np.where(c2, r - one, np.where(c3, r - h, -one)))
        den = np.where(c1, two + r, np.where(c2, r + one, np.where(c3, one + h * r, r)))
        t = np.where(c0, r, num / den)
        hi = np.where(c1, ATAN_HI[0], np.where(c2, ATAN_HI[1], np.where(c3, ATAN_HI[2], ATAN_HI[3])))
        lo = np.where(c1, ATAN_LO[0], np.where(c2, ATAN_LO[1], np.where(c3, ATAN_LO[2], ATAN_LO[3])))
        z = t * t
        w = z * z
        s1 = z * (T[0] + w * (T[2] + w * (T[4] + w * (T[6] + w * (T[8] + w * T[10])))))
        s2 = w * (T[1] + w * (T[3] + w * (T[5] + w * (T[7] + w * T[9]))))
        p = t * (s1 + s2)
        out = np.where(c0, t - p, hi - ((p - lo) - t))
        out = np.where(r >= ATAN_BIG, ATAN_HI[3], out)
        out = np.where(np.isnan(r), _F(np.nan), out)
    return out


def lens_map(rows, cols, model, K, coeffs, iR=None):
    """-> (iu, iv) int64 [rows, cols]: the source position of every destination pixel in 1/32 pixel"""
    model = int(model)
    if model == RADTAN:
        return um.undistort_map(rows, cols, K, coeffs, iR)
    if model != KB4:
        raise ValueError(REASONS["model"])
    fx, fy, cx, cy = (_F(v) for v in K)
    k1, k2, k3, k4 = (_F(v) for v in tuple(coeffs)[:4])
    iR = um.default_iR(K) if iR is None else np.asarray(iR, dtype=np.float64).reshape(9)
    j = np.arange(cols, dtype=np.float64)[None, :]
    i = np.arange(rows, dtype=np.float64)[:, None]
    one = _F(1.0)
    with np.errstate(all="ignore"):
        X = (j * iR[0] + i * iR[1]) + iR[2]
        Y = (j * iR[3] + i * iR[4]) + iR[5]
        W = (j * iR[6] + i * iR[7]) + iR[8]
        w = one / W
        x = X * w
        y = Y * w
        r2 = x * x + y * y
        r = np.sqrt(r2)
        th = atan_c(r)
        t2 = th * th
        thd = th * (one + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        s = np.where(r == 0, one, thd / r)
        u = fx * (x * s) + cx
        v = fy * (y * s) + cy
        front = W > 0
        u = np.where(front, u, -np.inf)
        v = np.where(front, v, -np.inf)
        iu = um._q(u * _F(32.0))
        iv = um._q(v * _F(32.0))
    return iu, iv


def rectify_image(img, model, K, coeffs, iR):
    """the contract of ssx_undistort_lens for one image"""
    img = np.asarray(img)
    return um.remap(img, *lens_map(img.shape[0], img.shape[1], model, K, coeffs, iR))


def _iR(S, f, cx, cy):
    g, mx, my = _F(1.0) / f, -cx / f, -cy / f
    out = np.empty(9, dtype=np.float64)
    for i in range(3):
        out[3 * i + 0] = S[0][i] * g
        out[3 * i + 1] = S[1][i] * g
        out[3 * i + 2] = (S[0][i] * mx + S[1][i] * my) + S[2][i]
    return out


def rectify(rig):
    """rig = dict(cam=[dict(model=, K=(fx, fy, cx, cy), coeffs=), the same for the right camera], R=3x3, t=3, and optionally f=, cx=, cy=
    (None or 0: the default)) -> dict(R_l, R_r [3, 3], newK (4), b, iR_l, iR_r (9)), all float64"""
    cams = rig["cam"]
    for cam in cams:
        if int(cam["model"]) not in (RADTAN, KB4):
            raise ValueError(REASONS["model"])
    R = np.asarray(rig["R"], dtype=np.float64).reshape(3, 3)
    t = np.asarray(rig["t"], dtype=np.float64).reshape(3)
    Ks = [np.asarray(cam["K"], dtype=np.float64).reshape(4) for cam in cams]
    over = [_F(0.0) if rig.get(k) is None else _F(rig[k]) for k in ("f", "cx", "cy")]
    coeffs = [np.asarray(list(cam["coeffs"]) + [0.0] * (5 - len(cam["coeffs"])), dtype=np.float64) for cam in cams]
    if not all(np.isfinite(v).all() for v in (R, t, Ks[0], Ks[1], np.array(over), coeffs[0], coeffs[1])):
        raise ValueError(REASONS["finite"])
    with np.errstate(all="ignore"):
        c = [((-R[0][i]) * t[0] + (-R[1][i]) * t[1]) + (-R[2][i]) * t[2] for i in range(3)]
        b = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        if b == 0:
            raise ValueError(REASONS["baseline"])
        worst = _F(0.0)
        for i in range(3):
            for j in range(3):
                dev = abs(((R[i][0] * R[j][0] + R[i][1] * R[j][1]) + R[i][2] * R[j][2]) - _F(1.0 if i == j else 0.0))
                worst = dev if dev > worst else worst
        if worst > _F(1e-6):
            raise ValueError(REASONS["rotation"])
        e1 = [c[i] / b for i in range(3)]
        if e1[0] <= 0:
            raise ValueError(REASONS["side"])
        zm = [_F(0.0) + R[2][0], _F(0.0) + R[2][1], _F(1.0) + R[2][2]]
        d = (zm[0] * e1[0] + zm[1] * e1[1]) + zm[2] * e1[2]
        e3p = [zm[i] - d * e1[i] for i in range(3)]
        n2 = (e3p[0] * e3p[0] + e3p[1] * e3p[1]) + e3p[2] * e3p[2]
        if n2 < _F(1e-12):
            raise ValueError(REASONS["axes"])
        n = np.sqrt(n2)
        e3 = [e3p[i] / n for i in range(3)]
        e2 = [e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]]
        R_l = np.array([e1, e2, e3], dtype=np.float64)
        R_r = np.empty((3, 3), dtype=np.float64)
        for i in range(3):
            for j in range(3):
                R_r[i][j] = (R_l[i][0] * R[j][0] + R_l[i][1] * R[j][1]) + R_l[i][2] * R[j][2]
        f = over[0] if over[0] != 0 else ((Ks[0][0] + Ks[0][1]) + (Ks[1][0] + Ks[1][1])) / _F(4.0)
        cx = over[1] if over[1] != 0 else (Ks[0][2] + Ks[1][2]) / _F(2.0)
        cy = over[2] if over[2] != 0 else (Ks[0][3] + Ks[1][3]) / _F(2.0)
        return dict(R_l=R_l, R_r=R_r, newK=np.array([f, f, cx, cy], dtype=np.float64), b=_F(b), iR_l=_iR(R_l, f, cx, cy), iR_r=_iR(R_r, f, cx, cy))


# ---- test inputs: not part of the contract ----

def rot(rx, ry, rz):
    """Rz(rz) Ry(ry) Rx(rx), radians (test inputs only)"""
    cxr, sxr, cyr, syr, czr, szr = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cxr, -sxr], [0, sxr, cxr]])
    Ry = np.array([[cyr, 0, syr], [0, 1, 0], [-syr, 0, cyr]])
    Rz = np.array([[czr, -szr, 0], [szr, czr, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def atan_sweep(n=3000, seed=7):
    """the fixed arguments atan_c is tested on (test inputs only): n uniform in [0, 3], n log-uniform over 1e-12 .. 1e12, the four
    breakpoints with their neighbours, and 0, 2^66 with its neighbours, 1e300, inf, NaN"""
    rng = np.random.default_rng(seed)
    brk = np.array([0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66])
    edge = np.concatenate([brk, np.nextafter(brk, 0.0), np.nextafter(brk, np.inf), [0.0, 2.0 ** -29, 1.0, 1e300, np.inf, np.nan]])
    return np.concatenate([rng.uniform(0.0, 3.0, n), 10.0 ** rng.uniform(-12.0, 12.0, n), edge]).astype(np.float64)


def rig_share(rows, cols, iu, iv):
    """-> (inside, none, partial): the shares of a map's pixels with all four taps inside the image, none, and some (test inputs only)"""
    inside = um.all_taps_inside(rows, cols, iu, iv)
    X0, Y0 = iu >> 5, iv >> 5
    none = (X0 < -1) | (X0 >= cols) | (Y0 < -1) | (Y0 >= rows)
    return float(inside.mean()), float(none.mean()), float((~inside & ~none).mean())


def unrectify_image(img, newK, R_side, model, K, coeffs, iters=20):
    """Forward warp (test inputs only): the image the raw camera (model, K, coeffs), whose rectifying rotation is R_side, would have
    taken of what `img` shows in the rectified camera newK.  Every pixel of the result is a raw position; the lens is inverted in f64
    (radtan: `iters` fixed-point iterations; kb4: `iters` Newton steps on theta), the ray is rotated into the rectified frame and `img`
    is sampled bilinearly in float there (clamped at the border), rounded to nearest."""
    img = np.asarray(img)
    rows, cols = img.shape
    fx, fy, cx, cy = (float(v) for v in K)
    nf, _, ncx, ncy = (float(v) for v in newK)
    jj, ii = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    xd, yd = (jj - cx) / fx, (ii - cy) / fy
    if int(model) == RADTAN:
        k1, k2, p1, p2, k3 = (list(float(v) for v in coeffs) + [0.0] * 5)[:5]
        x, y = xd.copy(), yd.copy()
        for _ in range(int(iters)):
            r2 = x * x + y * y
            kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (xd - dx) / kr, (yd - dy) / kr
    else:
        k1, k2, k3, k4 = (float(v) for v in tuple(coeffs)[:4])
        rd = np.sqrt(xd * xd + yd * yd)
        th = rd.copy()
        for _ in range(int(iters)):
            t2 = th * th
            g = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - rd
            dg = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4)))
            th = th - g / dg
        s = np.where(rd > 0, np.tan(th) / np.where(rd > 0, rd, 1.0), 1.0)
        x, y = xd * s, yd * s
    Rs = np.asarray(R_side, dtype=np.float64).reshape(3, 3)
    X = Rs[0, 0] * x + Rs[0, 1] * y + Rs[0, 2]
    Y = Rs[1, 0] * x + Rs[1, 1] * y + Rs[1, 2]
    Z = Rs[2, 0] * x + Rs[2, 1] * y + Rs[2, 2]
    u = np.clip(nf * X / Z + ncx, 0.0, cols - 1.0)
    v = np.clip(nf * Y / Z + ncy, 0.0, rows - 1.0)
    x0 = np.minimum(np.floor(u).astype(np.int64), cols - 2)
    y0 = np.minimum(np.floor(v).astype(np.int64), rows - 2)
    a, b = (u - x0).astype(np.float32), (v - y0).astype(np.float32)
    f = img.astype(np.float32)
    one = np.float32(1.0)
    val = (one - b) * ((one - a) * f[y0, x0] + a * f[y0, x0 + 1]) + b * ((one - a) * f[y0 + 1, x0] + a * f[y0 + 1, x0 + 1])
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)
