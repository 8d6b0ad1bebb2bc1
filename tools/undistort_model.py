"""The contract of image undistortion, in plain numpy (the style of tools/pnp_model.py): what ssx_undistort (csrc/undistort.hip:
k_undistort) writes for Camera::UndistortImage (camera.cpp:43-55, a cv::undistort with the camera matrix and k1 k2 p1 p2).

OpenCV cannot be pinned here, so the contract restates cv::undistort's arithmetic as far as it can be stated without it: a map
quantised to 1/32 pixel, integer bilinear weights, a constant border of 0.  For the destination pixel (row i, column j) of a
rows x cols image, with K = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3) and iR = the inverse of newK * R, row-major:

    X = (j*iR[0] + i*iR[1]) + iR[2];  Y = (j*iR[3] + i*iR[4]) + iR[5];  W = (j*iR[6] + i*iR[7]) + iR[8]
    w = 1/W;  x = X*w;  y = Y*w
    x2 = x*x; y2 = y*y; r2 = x2 + y2; _2xy = (2*x)*y
    kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
    xd = (x*kr + p1*_2xy) + p2*(r2 + 2*x2)
    yd = (y*kr + p1*(r2 + 2*y2)) + p2*_2xy
    u = fx*xd + cx;  v = fy*yd + cy
    iu = q(u*32), iv = q(v*32)     q(t) = 0 if t is NaN, else rint(t) (ties to even) clamped to [-2^31, 2^31 - 1]
    X0 = iu >> 5, Y0 = iv >> 5 (arithmetic shifts), a = iu & 31, b = iv & 31
    out = ((32-a)(32-b)*p(Y0,X0) + a(32-b)*p(Y0,X0+1) + (32-a)b*p(Y0+1,X0) + ab*p(Y0+1,X0+1) + 512) >> 10

Everything up to q is f64, every operation rounded on its own in the order written (no fused multiply-add).  p(Y, X) is the source
byte, or 0 for each tap on its own when that tap lies outside [0, rows) x [0, cols); the test is made on the integer coordinates.
A non-finite or far-away coordinate is an ordinary case and raises nothing: +-inf and anything beyond +-2^26 pixels clamp to
positions whose four taps are outside, so the pixel is 0; a NaN coordinate quantises to 0 by q's first case (the position 0 on that
axis, a position like any other).

Deviations from OpenCV:
  * rows are evaluated in closed form (j*iR[0] + ...); OpenCV accumulates _x += ir[0] along a row and works in stripes;
  * the weights are the 10-bit products of the 5-bit fractions; OpenCV reads them from its 15-bit table -- equal results wherever
    that table is exact;
  * the integer position is never narrowed to 16 bits (OpenCV's CV_16SC2 map).

default_iR(K) = [1/fx, 0, -cx/fx, 0, 1/fy, -cy/fy, 0, 0, 1] is the reference's case: R = I, new camera matrix = the old one.

distort_image is NOT part of the contract: the forward warp that makes distorted test inputs from rectified images."""
import numpy as np

INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1


def default_iR(K):
    fx, fy, cx, cy = (np.float64(v) for v in K)
    one, zero = np.float64(1.0), np.float64(0.0)
    return np.array([one / fx, zero, -cx / fx, zero, one / fy, -cy / fy, zero, zero, one], dtype=np.float64)


def _q(t):
    """NaN -> 0, else rint (ties to even) clamped to int32"""
    t = np.where(np.isnan(t), 0.0, t)
    with np.errstate(invalid="ignore"):
        r = np.rint(t)
    r = np.clip(r, float(INT32_MIN), float(INT32_MAX))          # both bounds are doubles; +-inf clamps
    return r.astype(np.int64)


def undistort_map(rows, cols, K, dist, iR=None):
    """-> (iu, iv) int64 [rows, cols]: the source position of every destination pixel in 1/32 pixel"""
    fx, fy, cx, cy = (np.float64(v) for v in K)
    k1, k2, p1, p2, k3 = (np.float64(v) for v in dist)
    iR = default_iR(K) if iR is None else np.asarray(iR, dtype=np.float64).reshape(9)
    j = np.arange(cols, dtype=np.float64)[None, :]
    i = np.arange(rows, dtype=np.float64)[:, None]
    two = np.float64(2.0)
    with np.errstate(all="ignore"):
        X = (j * iR[0] + i * iR[1]) + iR[2]
        Y = (j * iR[3] + i * iR[4]) + iR[5]
        W = (j * iR[6] + i * iR[7]) + iR[8]
        w = np.float64(1.0) / W
        x = X * w
        y = Y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = (two * x) * y
        kr = np.float64(1.0) + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * _2xy) + p2 * (r2 + two * x2)
        yd = (y * kr + p1 * (r2 + two * y2)) + p2 * _2xy
        u = fx * xd + cx
        v = fy * yd + cy
        iu = _q(u * np.float64(32.0))
        iv = _q(v * np.float64(32.0))
    return iu, iv


def remap(img, iu, iv):
    """the integer bilinear sample of img at (iu, iv) / 32, taps outside the image reading 0"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("an 8-bit single-channel image")
    rows, cols = img.shape
    X0, Y0 = iu >> 5, iv >> 5
    a, b = iu & 31, iv & 31

    def p(Y, X):
        inside = (Y >= 0) & (Y < rows) & (X >= 0) & (X < cols)
        return np.where(inside, img[np.clip(Y, 0, rows - 1), np.clip(X, 0, cols - 1)], 0).astype(np.int64)

    acc = (32 - a) * (32 - b) * p(Y0, X0) + a * (32 - b) * p(Y0, X0 + 1) + (32 - a) * b * p(Y0 + 1, X0) + a * b * p(Y0 + 1, X0 + 1)
    return ((acc + 512) >> 10).astype(np.uint8)


def undistort(img, K, dist, iR=None):
    """-> uint8 [rows, cols]: the contract of ssx_undistort for one image"""
    img = np.asarray(img)
    iu, iv = undistort_map(img.shape[0], img.shape[1], K, dist, iR)
    return remap(img, iu, iv)


MAP_MAX_SIDE = 65533                      # the stored position + 2 must fit a u16: side + 2 <= 65535


def pack_map(rows, cols, iu, iv):
    """The stored form of a map (ssx_undistort_plan, csrc/undistort.hip: k_undistort_map): -> (xs, ys, ab), three uint16 [rows, cols].
    With X0 = iu >> 5, Y0 = iv >> 5, a = iu & 31, b = iv & 31: X0 clamped to [-2, cols] and Y0 to [-2, rows], then
    xs = X0 + 2, ys = Y0 + 2, ab = a | b << 5.  The clamp keeps every tap's inside / outside test: at -2 both taps of the axis (-2, -1)
    are outside as they are anywhere below, at `cols` (`rows`) both are outside as they are anywhere above; a pixel whose taps are
    all outside is 0 whatever its fractions are."""
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1 or rows > MAP_MAX_SIDE or cols > MAP_MAX_SIDE:
        raise ValueError("pack_map: %d x %d: a side is 1 .. %d" % (rows, cols, MAP_MAX_SIDE))
    iu, iv = np.asarray(iu, dtype=np.int64), np.asarray(iv, dtype=np.int64)
    if iu.shape != (rows, cols) or iv.shape != (rows, cols):
        raise ValueError("pack_map: iu and iv are [rows, cols]")
    X0 = np.clip(iu >> 5, -2, cols)
    Y0 = np.clip(iv >> 5, -2, rows)
    return (X0 + 2).astype(np.uint16), (Y0 + 2).astype(np.uint16), ((iu & 31) | ((iv & 31) << 5)).astype(np.uint16)


def unpack_map(xs, ys, ab):
    """-> (iu', iv') int64 with remap(img, iu', iv') == remap(img, iu, iv) for every image of the map's size"""
    xs, ys, ab = (np.asarray(v).astype(np.int64) for v in (xs, ys, ab))
    return ((xs - 2) << 5) | (ab & 31), ((ys - 2) << 5) | ((ab >> 5) & 31)


def clamped_share(rows, cols, iu, iv):
    """the share of a map's pixels whose integer position pack_map's clamp changes"""
    X0, Y0 = np.asarray(iu) >> 5, np.asarray(iv) >> 5
    return float(((X0 < -2) | (X0 > cols) | (Y0 < -2) | (Y0 > rows)).mean())


def all_taps_inside(rows, cols, iu, iv):
    X0, Y0 = iu >> 5, iv >> 5
    return (X0 >= 0) & (X0 + 1 < cols) & (Y0 >= 0) & (Y0 + 1 < rows)


def rotated_iR(K, rx, ry, rz, newK=None):
    """inverse of newK * R with R = Rz(rz) Ry(ry) Rx(rx) (radians), newK = K by default: a general iR for the tests (W != 1)"""
    fx, fy, cx, cy = (float(v) for v in K)
    nfx, nfy, ncx, ncy = (float(v) for v in (K if newK is None else newK))
    cxr, sxr, cyr, syr, czr, szr = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cxr, -sxr], [0, sxr, cxr]])
    Ry = np.array([[cyr, 0, syr], [0, 1, 0], [-syr, 0, cyr]])
    Rz = np.array([[czr, -szr, 0], [szr, czr, 0], [0, 0, 1]])
    A = np.array([[nfx, 0, ncx], [0, nfy, ncy], [0, 0, 1]]) @ (Rz @ Ry @ Rx)
    return np.linalg.inv(A).reshape(9).astype(np.float64)


def distort_image(img, K, dist, iters=20):
    """Forward warp (test inputs only): the image a camera with `dist` would have taken of what `img` shows rectified.  Every pixel of the
    result is a distorted position; the distortion is inverted by `iters` fixed-point iterations in f64 and `img` is sampled
    bilinearly in float there (clamped at the border), rounded to nearest."""
    img = np.asarray(img)
    rows, cols = img.shape
    fx, fy, cx, cy = (float(v) for v in K)
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    jj, ii = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    xd, yd = (jj - cx) / fx, (ii - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(int(iters)):
        r2 = x * x + y * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) / kr, (yd - dy) / kr
    u = np.clip(fx * x + cx, 0.0, cols - 1.0)
    v = np.clip(fy * y + cy, 0.0, rows - 1.0)
    x0 = np.minimum(np.floor(u).astype(np.int64), cols - 2)
    y0 = np.minimum(np.floor(v).astype(np.int64), rows - 2)
    a, b = (u - x0).astype(np.float32), (v - y0).astype(np.float32)
    f = img.astype(np.float32)
    one = np.float32(1.0)
    val = (one - b) * ((one - a) * f[y0, x0] + a * f[y0, x0 + 1]) + b * ((one - a) * f[y0 + 1, x0] + a * f[y0 + 1, x0 + 1])
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)
