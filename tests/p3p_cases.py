"""The inputs of tests/golden/p3p_hp.npz (tests/golden/make_p3p_hp.py solves them to 60 digits; tests/test_p3p_cases.py and
tests/test_p3p_gpu.py hold tools/pnp_model.py::p3p and the kernel's p3p_solve to that reference).  A case is three world points X, their
three pixels uv and the pose (R, t) that generated them: camera-frame points pc are chosen first, X = R' (pc - t) and
uv = K pc / pc_z are computed in double, and those doubles ARE the problem -- the generating pose solves it only to rounding, which is
why the reference, not the generating pose, is the yardstick.

Classes:
  baseline     KITTI-like triples, pose near identity
  rotation     the first baseline triples under rotations that take each branch of rot_to_quat (asserted here per case)
  far-world    the world origin 1e2 .. 1e5 m away: t = Y0 - R X0 cancels
  shape        special triangles and viewing geometries
  behind       the generating pose puts one or two points behind the camera
  random-any   rotation angle uniform in [0, pi], translation up to 3 m
  ill-posed    near-collinear, collinear, repeated point / bearing, the danger cylinder, NaN and inf
"""
import os

import numpy as np

from tools.synth import KITTI_H, KITTI_K, KITTI_W

K = np.array(KITTI_K, dtype=np.float64)
CLASSES = ("baseline", "rotation", "far-world", "shape", "behind", "random-any", "ill-posed")
BROAD = ("baseline", "rotation", "far-world", "random-any")       # at least 80 % of each is well-posed
NEAR_COLLINEAR_E = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)
FAR_OFFSETS = (1e2, 1e3, 1e4, 1e5)
PROBE_ROTVEC = (0.2, 0.1, 0.3)                                     # the pose of the near-collinear family
PROBE_T = (1.0, 0.0, 0.0)


def rodrigues(axis, angle):
    """rotation matrix; sines and cosines within 1e-15 of 0 are taken as 0, so 90 and 180 degrees about a coordinate axis are exact"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    c, s = np.cos(angle), np.sin(angle)
    c = 0.0 if abs(c) < 1e-15 else c
    s = 0.0 if abs(s) < 1e-15 else s
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return c * np.eye(3) + s * Kx + (1 - c) * np.outer(a, a)


def rotvec(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    return np.eye(3) if th == 0 else rodrigues(w / th, th)


def quat_branch(R):
    """which branch of rot_to_quat R takes: 0 trace > 0, 1 / 2 / 3 the largest diagonal entry is xx / yy / zz"""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return 1
    return 2 if R[1, 1] > R[2, 2] else 3


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def from_camera(pc, R, t):
    """(X, uv) of camera-frame points pc under the pose x_cam = R X + t"""
    pc = np.asarray(pc, dtype=np.float64).reshape(3, 3)
    X = (pc - np.asarray(t, dtype=np.float64)) @ R                  # rows: R' (pc_i - t)
    uv = np.stack([K[0] * (pc[:, 0] / pc[:, 2]) + K[2], K[1] * (pc[:, 1] / pc[:, 2]) + K[3]], 1)
    return np.ascontiguousarray(X), np.ascontiguousarray(uv)


def _kitti_pc(rng):
    uv = np.stack([rng.uniform(20, KITTI_W - 20, 3), rng.uniform(20, KITTI_H - 20, 3)], 1)
    d = rng.uniform(6, 45, 3)
    return np.stack([(uv[:, 0] - K[2]) / K[0] * d, (uv[:, 1] - K[3]) / K[1] * d, d], 1)


def _near_identity(rng):
    w = rng.uniform(0.03, 0.08, 3) * rng.choice([-1.0, 1.0], 3)
    return rotvec(w), rng.uniform(1.0, 3.0, 3) * rng.choice([-1.0, 1.0], 3)


def _rotations():
    """(name, R, expected branch or None) of the rotation class"""
    out = []
    for ax, e in zip("xyz", np.eye(3)):
        for name, ang in (("90", np.pi / 2), ("120", 2 * np.pi / 3), ("170", np.deg2rad(170.0)), ("180-1e-3", np.pi - np.deg2rad(1e-3)),
                          ("180", np.pi)):
            out.append((f"{ax}{name}", rodrigues(e, ang), None))
    out.append(("111-120", np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]), 3))          # the trace is exactly 0, no diagonal entry exceeds another
    out.append(("111-2rad", rodrigues((1, 1, 1), 2.0), None))
    rng = np.random.default_rng(4100)
    for k in range(12):
        out.append((f"rand{k}", rodrigues(rng.normal(size=3), rng.uniform(2.0, np.pi)), None))
    return out


def _build():
    cases = []

    def add(cls, name, pc, R, t, X=None, uv=None):
        if X is None:
            X, uv = from_camera(pc, R, t)
        cases.append(dict(cls=cls, name=f"{cls}/{name}", X=np.array(X, dtype=np.float64), uv=np.array(uv, dtype=np.float64),
                          R=np.array(R, dtype=np.float64), t=np.array(t, dtype=np.float64)))

    rng = np.random.default_rng(4000)
    base_pc = []
    for k in range(100):
        pc = _kitti_pc(rng)
        R, t = _near_identity(rng)
        base_pc.append((pc, t))
        add("baseline", str(k), pc, R, t)

    branches = np.zeros(4, int)
    for name, R, want in _rotations():
        b = quat_branch(R)
        assert want is None or b == want, (name, b)
        if name[0] in "xyz" and name[1:] in ("170", "180-1e-3", "180"):
            assert b == 1 + "xyz".index(name[0]), (name, b)
        if name[1:] == "90" or name == "111-2rad":
            assert b == 0, (name, b)
        for k in range(2):
            pc, t = base_pc[k]
            add("rotation", f"{name}-{k}", pc, R, t)
            branches[b] += 1
    assert (branches >= 10).all(), branches

    Rp = rotvec(PROBE_ROTVEC)
    rng = np.random.default_rng(4200)
    for off in FAR_OFFSETS:
        for k in range(5):
            add("far-world", f"{off:g}-{k}", _kitti_pc(rng), Rp, (off, -off, off / 2))

    poses = (("id", np.eye(3), (0.0, 0.0, 0.0)), ("probe", Rp, PROBE_T))
    c30, s30 = np.cos(np.pi / 6), np.sin(np.pi / 6)
    tri = np.array([[0.0, 1.0, 0.0], [-c30, -s30, 0.0], [c30, -s30, 0.0]])           # equilateral, circumradius 1
    shapes = []
    for d in (5.0, 50.0):
        shapes.append((f"equilateral-on-axis-{d:g}", tri + [0, 0, d]))
        shapes.append((f"equilateral-off-axis-{d:g}", tri + [1e-3 * d, 0, d]))
    shapes += [("isosceles", [[-1.0, 0, 10], [1, 0, 10], [0, 3, 12]]),
               ("on-principal-axis", [[0.0, 0, 8], [3, -1, 14], [-2, 1.5, 9]]),
               ("mirror-bearings", [[-2.0, 1, 10], [2, 1, 10], [0.3, -1, 7]]),
               ("depths-1-30-500", [[0.2, 0.1, 1], [-9, 2, 30], [120, -40, 500]]),
               ("1cm-at-50m", [[1.0, 0.5, 50], [1.01, 0.5, 50.002], [1.004, 0.509, 49.997]]),
               ("bearings-80-degrees", [[-8.39, 0, 10], [8.39, 0.5, 10], [0, 6, 9]]),
               ("fronto-parallel", [[-3.0, -1, 20], [2, -2, 20], [1, 3, 20]])]
    for sname, pc in shapes:
        for pname, R, t in poses:
            add("shape", f"{sname}-{pname}", np.array(pc, dtype=np.float64), R, t)

    rng = np.random.default_rng(4300)
    for k in range(8):
        pc = _kitti_pc(rng)
        pc[: 1 + k % 2] *= -1.0                                                     # one or two of the three behind the camera
        R, t = _near_identity(rng)
        add("behind", str(k), pc, R, t)

    rng = np.random.default_rng(4400)
    for k in range(100):
        R = rodrigues(rng.normal(size=3), rng.uniform(0.0, np.pi))
        d = rng.normal(size=3)
        add("random-any", str(k), _kitti_pc(rng), R, d / np.linalg.norm(d) * rng.uniform(0.0, 3.0))

    for e in NEAR_COLLINEAR_E:
        add("ill-posed", f"near-collinear-{e:g}", [[-2.0, 0, 10], [0, e, 10], [2, 0, 10]], Rp, PROBE_T)
    add("ill-posed", "collinear", [[-2.0, 0, 10], [0, 0, 10], [2, 0, 10]], Rp, PROBE_T)
    X, uv = from_camera([[-2.0, 0, 10], [1, 1, 12], [2, 0, 10]], Rp, PROBE_T)
    add("ill-posed", "repeated-point", None, Rp, PROBE_T, X[[0, 0, 1]], uv[[0, 0, 1]])
    add("ill-posed", "one-bearing-three-times", None, Rp, PROBE_T, X, uv[[0, 0, 0]])
    ang = np.deg2rad([100.0, 200.0, 300.0])
    for delta in (1e-3, 1e-6, 0.0):
        # a triangle of circumradius 2 in the plane z = 10 whose circumscribed cylinder (axis along z) passes within 2 delta of the camera centre
        pc = np.stack([2.0 * (1 + delta) + 2.0 * np.cos(ang), 2.0 * np.sin(ang), np.full(3, 10.0)], 1)
        add("ill-posed", f"danger-cylinder-{delta:g}", pc, Rp, PROBE_T)
        add("ill-posed", f"danger-cylinder-tilted-{delta:g}", pc @ rotvec((0.3, -0.2, 0.1)).T, Rp, PROBE_T)
    X, uv = from_camera([[-2.0, 1, 10], [1, 1, 12], [2, 0, 10]], Rp, PROBE_T)
    for name, i, v in (("nan-in-X", 0, np.nan), ("inf-in-X", 4, np.inf), ("nan-in-z", 9, np.nan), ("inf-in-z", 12, -np.inf)):
        Xb, ub = X.copy(), uv.copy()
        (Xb if i < 9 else ub).flat[i % 9] = v
        add("ill-posed", name, None, Rp, PROBE_T, Xb, ub)
    return cases


_CASES = None


def cases():
    """the list of dict(cls, name, X [3, 3], uv [3, 2], R [3, 3], t [3]); built once, read-only"""
    global _CASES
    if _CASES is None:
        _CASES = _build()
        for c in _CASES:
            for k in ("X", "uv", "R", "t"):
                c[k].setflags(write=False)
    return _CASES


def arrays():
    """-> cls [N] (index into CLASSES), names [N], X [N, 3, 3], uv [N, 3, 2], R [N, 3, 3], t [N, 3]"""
    cs = cases()
    return (np.array([CLASSES.index(c["cls"]) for c in cs], np.int32), np.array([c["name"] for c in cs]), np.stack([c["X"] for c in cs]),
            np.stack([c["uv"] for c in cs]), np.stack([c["R"] for c in cs]), np.stack([c["t"] for c in cs]))


# ---- the fixture and what is asserted against it (shared by tests/test_p3p_cases.py, tests/test_p3p_gpu.py and the generator) ----

REPROJ_PX = 0.01 * 5.991                 # a hypothesis explains its own sample at a hundredth of the inlier threshold


def load(path):
    """tests/golden/p3p_hp.npz as a dict; R [N, 4, 3, 3] is the rotation of the stored 60-digit quaternion (the file holds q: 4 numbers
    instead of 9; turning its double back into a matrix costs < 1e-15, against bars that start at 1e-9)"""
    with np.load(path) as z:
        fx = {k: z[k] for k in z.files}
    fx["R"] = np.zeros(fx["q"].shape[:2] + (3, 3))
    for i in range(len(fx["n"])):
        for s in range(fx["n"][i]):
            fx["R"][i, s] = quat_to_rot(fx["q"][i, s])
    fx["xmax"] = np.array([np.abs(x).max() if np.isfinite(x).all() else 1.0 for x in fx["X"]])
    return fx


def case_err(R, t, R_ref, t_ref, xmax):
    """the error of a solution against a reference solution: max(max |R - R_ref|, |t - t_ref| / max(1, |X|max))"""
    return max(np.abs(R - R_ref).max(), np.linalg.norm(t - t_ref) / max(1.0, xmax))


def match(valid, Rs, ts, ref_n, ref_R, ref_t, xmax):
    """greedy one-to-one matching of the valid slots to the reference solutions by case_err -> (pairs [(slot, ref, err)], unmatched slots,
    unmatched reference solutions)"""
    slots, refs = [int(s) for s in np.nonzero(valid)[0]], list(range(int(ref_n)))
    cand = sorted((case_err(Rs[s], ts[s], ref_R[r], ref_t[r], xmax), s, r) for s in slots for r in refs)
    pairs = []
    for e, s, r in cand:
        if s in slots and r in refs:
            pairs.append((s, r, e))
            slots.remove(s)
            refs.remove(r)
    return pairs, slots, refs


def own_sample(Kd, X, uv, pose):
    """the pose that is handed on (qx qy qz qw tx ty tz) against the triple it came from, in exact rational arithmetic on the doubles ->
    (smallest depth, largest reprojection error in px) as floats"""
    from fractions import Fraction as Q
    x, y, z, w, tx, ty, tz = (Q(float(v)) for v in pose)
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    fx, fy, cx, cy = (Q(float(v)) for v in Kd)
    zmin, e2max = None, Q(0)
    for i in range(3):
        P = [Q(float(v)) for v in X[i]]
        c = [R[a][0] * P[0] + R[a][1] * P[1] + R[a][2] * P[2] + t for a, t in zip(range(3), (tx, ty, tz))]
        zmin = c[2] if zmin is None else min(zmin, c[2])
        if c[2] <= 0:
            return float(zmin), float("inf")
        ex, ey = fx * c[0] / c[2] + cx - Q(float(uv[i][0])), fy * c[1] / c[2] + cy - Q(float(uv[i][1]))
        e2max = max(e2max, ex * ex + ey * ey)
    return float(zmin), float(e2max) ** 0.5


def check(fx, valid, R, t, pose, bar, zero_invalid, skip=()):
    """The conditions of a solver's output over the whole fixture, against the fixture alone.  valid [N, 4], R [N, 4, 3, 3], t [N, 4, 3],
    pose [N, 4, 7]; bar [classes].  Well-posed cases: the valid slots and the reference's solutions match one to one within the class
    bar.  Every case: a valid slot is finite, its pose a unit quaternion with qw >= 0 that explains its own triple (positive depths,
    REPROJ_PX).  A slot that is not valid is finite, and all zeros where zero_invalid.  -> worst error per class over the well-posed cases"""
    worst = np.zeros(len(fx["classes"]))
    for i in range(len(fx["n"])):
        name, c = str(fx["names"][i]), int(fx["cls"][i])
        v = valid[i].astype(bool)
        assert np.isfinite(R[i]).all() and np.isfinite(t[i]).all() and np.isfinite(pose[i]).all(), name
        for s in np.nonzero(~v)[0]:
            if zero_invalid:
                assert not R[i, s].any() and not t[i, s].any() and not pose[i, s].any(), (name, s)
        for s in np.nonzero(v)[0]:
            q = pose[i, s, :4]
            assert abs(np.sqrt((q * q).sum()) - 1.0) < 1e-14 and q[3] >= 0, (name, s, q)
            assert pose[i, s, 4:].tobytes() == t[i, s].tobytes(), (name, s)
            zmin, px = own_sample(fx["K"], fx["X"][i], fx["uv"][i], pose[i, s])
            assert zmin > 0 and px <= REPROJ_PX, (name, s, zmin, px)
        if fx["well"][i] and name not in skip:
            pairs, extra, missing = match(v, R[i], t[i], fx["n"][i], fx["R"][i], fx["t"][i], fx["xmax"][i])
            assert not extra and not missing, (name, "extra slots", extra, "missing reference solutions", missing)
            for s, r, e in pairs:
                assert e <= bar[c], (name, s, r, e, bar[c])
                worst[c] = max(worst[c], e)
    return worst


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p3p_hp.npz")
_CACHE = {}


def fixture():
    """the fixture, loaded once per session (read-only)"""
    if "fx" not in _CACHE:
        _CACHE["fx"] = load(FIXTURE)
    return _CACHE["fx"]


def model_output():
    """tools/pnp_model.py over the fixture's inputs, computed once per session -> valid [N, 4] int32, R [N, 4, 3, 3], t [N, 4, 3],
    pose [N, 4, 7] (rot_to_quat(R), t; zeros where the slot is not valid: what ssx_pnp_debug_p3p writes)"""
    if "model" not in _CACHE:
        from tools import pnp_model as pm
        fx = fixture()
        N = len(fx["n"])
        valid, R, t, pose = np.zeros((N, 4), np.int32), np.zeros((N, 4, 3, 3)), np.zeros((N, 4, 3)), np.zeros((N, 4, 7))
        for i in range(N):
            v, R[i], t[i] = pm.p3p(fx["K"], fx["X"][i], fx["uv"][i])
            valid[i] = v
            for s in np.nonzero(v)[0]:
                pose[i, s] = np.concatenate([pm.rot_to_quat(R[i, s]), t[i, s]])
        _CACHE["model"] = (valid, R, t, pose)
    return _CACHE["model"]
