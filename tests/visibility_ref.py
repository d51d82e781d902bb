"""TEST INFRASTRUCTURE: camera::countVisible (src/camera.cc:135-198) with camera::isInFrustum (:263-315), restated literally in
np.float32 scalars -- one state and one point at a time, cos / sin / atan2 as the float64 functions rounded to float32, a
sequential float32 sum, std::round's half-away rounding -- with StateValidChecker::MotionCostCamera (src/StateValidChecker.cc:531-541)
and plan_slam::AdvanceStepCamera (src/plan.cc:141-151) over its counts.  The operation order of the matrix product and of the 4x4
inverse is the one csrc/visibility.h writes down.  Also here: the seeded generator of the random
cases, the planted cases and the golden planner map, shared by the CPU and the GPU tests; a case is computed once per process."""
import functools
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FLT_MAX = np.finfo(np.float32).max
INT32_MIN = -2 ** 31
NEAR_ULPS = 4
# the returns of isInFrustum, by the half of the test that fires; 0 = success
OK, DEPTH, U_LOW, U_HIGH, V_LOW, V_HIGH, DIST_LOW, DIST_HIGH, RANGE_LOW, RANGE_HIGH, DIR_LOW, DIR_HIGH = range(12)


class Camera:
    def __init__(self, fx, fy, cx, cy, min_x, max_x, min_y, max_y, max_dist, min_dist, feature_threshold=20):
        self.fx, self.fy, self.cx, self.cy = F(fx), F(fy), F(cx), F(cy)
        self.min_x, self.max_x, self.min_y, self.max_y = F(min_x), F(max_x), F(min_y), F(max_y)
        self.max_dist, self.min_dist = F(max_dist), F(min_dist)
        self.feature_threshold = int(feature_threshold)
        # src/camera.cc:46-54
        self.T_sw = [F(v) for v in (0, -1, 0, -0.1, 0, 0, -1, 0, 1, 0, 0, -0.25, 0, 0, 0, 1)]
        self.T_bc = [F(v) for v in (0, 0, 1, 0.25, -1, 0, 0, -0.1, 0, -1, 0, 0, 0, 0, 0, 1)]

    def to_capi(self, pkg):
        c = pkg.VisCamera()
        for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "max_dist", "min_dist"):
            setattr(c, k, float(getattr(self, k)))
        c.feature_threshold = self.feature_threshold
        for i in range(16):
            c.T_sw[i], c.T_bc[i] = float(self.T_sw[i]), float(self.T_bc[i])
        return c


def camera_with_map():      # camera(map_data, int) :9-20
    return Camera(520.49, 522.47, 474.95, 264.27, 10, 930, 20, 520, 6, 0.5)


def camera_plain():         # camera() :109-120
    return Camera(520.49, 522.47, 474.95, 264.27, 10, 950, 10, 530, 6, 0.1)


def camera_exact(min_dist=0.5):
    """every constant exactly representable: with state (0, 0, 0), where T_sc = T_cs = I, u and v of the planted points are exact"""
    return Camera(512, 512, 480, 256, 32, 1024, 16, 512, 8, min_dist)


class Map:
    def __init__(self, xyz, upper, lower, max_range, min_range, ratio):
        self.xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.upper, self.lower, self.max_range, self.min_range, self.ratio = (
            np.ascontiguousarray(a, np.float32).reshape(-1) for a in (upper, lower, max_range, min_range, ratio))
        self.n = len(self.xyz)

    def rows(self):
        """the points as tuples of np.float32 scalars"""
        return list(zip(self.xyz[:, 0], self.xyz[:, 1], self.xyz[:, 2], self.upper, self.lower, self.max_range, self.min_range, self.ratio))

    def args(self):
        return self.xyz, self.upper, self.lower, self.max_range, self.min_range, self.ratio


# ---------------------------------------------------------------------------------------- the restatement
def mul44(A, B):
    """row-major 4x4: float products, float sums, ascending inner index"""
    C = [None] * 16
    for i in range(4):
        for j in range(4):
            s = A[4 * i] * B[j]
            for k in range(1, 4):
                s = s + A[4 * i + k] * B[4 * k + j]
            C[4 * i + j] = s
    return C


def inverse_rows(m):
    """rows 0..2 of the general 4x4 inverse by cofactors, in the operation order of csrc/visibility.h (vis_inverse_rows)"""
    s0, s1, s2 = m[0] * m[5] - m[4] * m[1], m[0] * m[6] - m[4] * m[2], m[0] * m[7] - m[4] * m[3]
    s3, s4, s5 = m[1] * m[6] - m[5] * m[2], m[1] * m[7] - m[5] * m[3], m[2] * m[7] - m[6] * m[3]
    c5, c4, c3 = m[10] * m[15] - m[14] * m[11], m[9] * m[15] - m[13] * m[11], m[9] * m[14] - m[13] * m[10]
    c2, c1, c0 = m[8] * m[15] - m[12] * m[11], m[8] * m[14] - m[12] * m[10], m[8] * m[13] - m[12] * m[9]
    det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0
    r = F(1) / det
    return [((m[5] * c5 - m[6] * c4) + m[7] * c3) * r, ((m[2] * c4 - m[1] * c5) - m[3] * c3) * r,
            ((m[13] * s5 - m[14] * s4) + m[15] * s3) * r, ((m[10] * s4 - m[9] * s5) - m[11] * s3) * r,
            ((m[6] * c2 - m[4] * c5) - m[7] * c1) * r, ((m[0] * c5 - m[2] * c2) + m[3] * c1) * r,
            ((m[14] * s2 - m[12] * s5) - m[15] * s1) * r, ((m[8] * s5 - m[10] * s2) + m[11] * s1) * r,
            ((m[4] * c4 - m[5] * c2) + m[7] * c0) * r, ((m[1] * c2 - m[0] * c4) - m[3] * c0) * r,
            ((m[12] * s4 - m[13] * s2) + m[15] * s0) * r, ((m[9] * s2 - m[8] * s4) - m[11] * s0) * r]


def pose_of(x, y, theta):
    """T_wb of countVisible(float, float, float) :142-146, row-major, as np.float32 scalars"""
    c, s = F(np.cos(np.float64(F(theta)))), F(np.sin(np.float64(F(theta))))
    return [c, -s, F(0), F(x), s, c, F(0), F(y), F(0), F(0), F(1), F(0), F(0), F(0), F(0), F(1)]


def state_from_pose(T_wb, cam):
    """-> (rows 0..2 of T_cs, T_sc(0,3), T_sc(2,3))  :148-149 / :180-181"""
    with np.errstate(all="ignore"):
        sc = mul44(mul44(cam.T_sw, [F(v) for v in T_wb]), cam.T_bc)
        return inverse_rows(sc), sc[3], sc[11]


def state_from_xyt(x, y, theta, cam):
    return state_from_pose(pose_of(x, y, theta), cam)


def is_in_frustum(cam, S, p):
    """:263-315 for the point p = (x, y, z, upper, lower, max_range, min_range, ...) -> which return it leaves by (OK = success)"""
    cs, sc03, sc23 = S
    x, y, z, upper, lower, max_range, min_range = p[:7]
    PcZ = ((cs[8] * x + cs[9] * y) + cs[10] * z) + cs[11]
    if PcZ < F(0.05):
        return DEPTH
    PcX = ((cs[0] * x + cs[1] * y) + cs[2] * z) + cs[3]
    PcY = ((cs[4] * x + cs[5] * y) + cs[6] * z) + cs[7]
    inv_z = F(1) / PcZ
    u = (cam.fx * PcX) * inv_z + cam.cx
    v = (cam.fy * PcY) * inv_z + cam.cy
    if u < cam.min_x:
        return U_LOW
    if u > cam.max_x:
        return U_HIGH
    if v < cam.min_y:
        return V_LOW
    if v > cam.max_y:
        return V_HIGH
    dist = np.sqrt((PcZ * PcZ + PcY * PcY) + PcX * PcX)
    if dist < cam.min_dist:
        return DIST_LOW
    if dist > cam.max_dist:
        return DIST_HIGH
    if dist < min_range:
        return RANGE_LOW
    if dist > max_range:
        return RANGE_HIGH
    theta = F(np.arctan2(np.float64(x - sc03), np.float64(z - sc23)))
    if theta < lower:
        return DIR_LOW
    if theta > upper:
        return DIR_HIGH
    return OK


def round_half_away(x):
    """int(round(float)) :166; out of int's range: INT32_MIN, the x86 conversion's answer"""
    t = np.trunc(x)
    if abs(x - t) >= F(0.5):
        t = t + np.copysign(F(1), x)
    return int(t) if -2.0 ** 31 <= float(t) < 2.0 ** 31 else INT32_MIN


def count_visible(cam, rows, S, n):
    """the loop :153-160 -> (count, num_visible, mask words, the return of every point)"""
    words = np.zeros((n + 63) // 64, np.uint64)
    codes = np.zeros(n, np.uint8)
    num_visible = F(0)
    with np.errstate(all="ignore"):
        for i, p in enumerate(rows):
            code = is_in_frustum(cam, S, p)
            codes[i] = code
            if code == OK:
                num_visible = num_visible + p[7]
                words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
        return round_half_away(num_visible), num_visible, words, codes


def motion_cost(counts, thr):
    """MotionCostCamera (src/StateValidChecker.cc:531-541) over the counts of ALL states of the motion Q"""
    C = np.float64(0)
    with np.errstate(all="ignore"):
        for i in range(1, len(counts) - 1):
            c = int(counts[i])
            C = C + (np.float64(1.) / np.float64(1e-4) if c < thr else np.float64(1.) / np.float64(c))
    return C


def advance_step(counts, thr):
    """AdvanceStepCamera (src/plan.cc:141-151)"""
    i = 0
    while i < len(counts) and counts[i] > thr:
        i += 1
    return i - 1


# ---------------------------------------------------------------------------------------- which pairs sit on a rounding boundary
def _near(q, thr):
    """|q - thr| <= NEAR_ULPS ulps of thr (the ulp above it; for FLT_MAX the one below)"""
    with np.errstate(all="ignore"):
        t = np.abs(np.asarray(thr, np.float32))
        up, down = np.spacing(t).astype(np.float64), (t - np.nextafter(t, F(0))).astype(np.float64)
        return np.abs(np.asarray(q, np.float64) - np.asarray(thr, np.float64)) <= NEAR_ULPS * np.where(np.isfinite(up), up, down)


def near_pairs(cam, m, states):
    """[ns][n] bool: a gate the point REACHES has its quantity within NEAR_ULPS float ulps of its threshold.  Vectorised float32
    with the restatement's operation order (+, *, /, sqrt are IEEE either way; the last bit of cos / sin / atan2 does not matter to a
    test against four ulps)."""
    out = np.zeros((len(states), m.n), bool)
    x, y, z = m.xyz[:, 0], m.xyz[:, 1], m.xyz[:, 2]
    with np.errstate(all="ignore"):
        for k, st in enumerate(states):
            cs, sc03, sc23 = state_from_xyt(st[0], st[1], st[2], cam)
            PcZ = ((cs[8] * x + cs[9] * y) + cs[10] * z) + cs[11]
            PcX = ((cs[0] * x + cs[1] * y) + cs[2] * z) + cs[3]
            PcY = ((cs[4] * x + cs[5] * y) + cs[6] * z) + cs[7]
            inv_z = F(1) / PcZ
            u, v = (cam.fx * PcX) * inv_z + cam.cx, (cam.fy * PcY) * inv_z + cam.cy
            dist = np.sqrt((PcZ * PcZ + PcY * PcY) + PcX * PcX)
            theta = np.arctan2((x - sc03).astype(np.float64), (z - sc23).astype(np.float64)).astype(np.float32)
            near = _near(PcZ, F(0.05))
            reach = ~(PcZ < F(0.05))
            for q, lo, hi in ((u, cam.min_x, cam.max_x), (v, cam.min_y, cam.max_y), (dist, cam.min_dist, cam.max_dist),
                              (dist, m.min_range, m.max_range), (theta, m.lower, m.upper)):
                near |= reach & (_near(q, lo) | _near(q, hi))
                reach &= ~((q < lo) | (q > hi))
            out[k] = near
    return out


# ---------------------------------------------------------------------------------------- cases
class Case:
    """a camera, a map and states with the restatement's answer for every state"""

    def __init__(self, cam, m, states, redrawn=0, drawn=0, replaced=0):
        self.cam, self.map = cam, m
        self.states = np.ascontiguousarray(states, np.float32).reshape(-1, 3)
        self.redrawn, self.drawn, self.replaced = redrawn, drawn, replaced
        rows = m.rows()
        res = [count_visible(cam, rows, state_from_xyt(s[0], s[1], s[2], cam), m.n) for s in self.states]
        self.count = np.array([r[0] for r in res], np.int32)
        self.sum = np.array([r[1] for r in res], np.float32)
        self.mask = np.array([r[2] for r in res], np.uint64).reshape(len(self.states), (m.n + 63) // 64)
        self.codes = np.array([r[3] for r in res], np.uint8).reshape(len(self.states), m.n)

    def poses(self):
        return np.array([pose_of(*s) for s in self.states], np.float32).reshape(-1, 16)

    def load(self, pkg, device=0):
        V = pkg.Visibility(device=device)
        V.set_camera(self.cam.to_capi(pkg))
        V.set_map(*self.map.args())
        return V


def draw_states(rng, ns):
    """x in [-2, 6], y in [-3, 3], theta in [-pi, pi]"""
    return np.stack([rng.uniform(-2, 6, ns), rng.uniform(-3, 3, ns), rng.uniform(-np.pi, np.pi, ns)], 1).astype(np.float32)


def draw_points(rng, n):
    """points of the map frame (z forward, x to the right, y down) around the states' area, with their bounds, ranges and ratios"""
    xyz = np.stack([rng.uniform(-5, 5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-4, 9, n)], 1)
    lower = rng.uniform(-np.pi, 0.5, n)
    upper = lower + rng.uniform(1.0, 4.0, n)
    return Map(xyz, upper, lower, rng.uniform(2, 9, n), rng.uniform(0, 1.5, n), rng.uniform(0.2, 1.0, n))


@functools.lru_cache(maxsize=None)
def random_case(seed, n, ns=300):
    """n random points against ns random states under the exact camera; a point with a near pair in any state is drawn again"""
    rng = np.random.default_rng(seed)
    cam = camera_exact()
    states = draw_states(rng, ns)
    m = draw_points(rng, n)
    drawn, redrawn = n, 0
    while n:
        bad = np.nonzero(near_pairs(cam, m, states).any(0))[0]
        if not len(bad):
            break
        fresh = draw_points(rng, len(bad))
        for a, b in zip(m.args(), fresh.args()):
            a[bad] = b
        drawn += len(bad)
        redrawn += len(bad)
    return Case(cam, m, states, redrawn, drawn)


def _map_of(points):
    a = np.array(points, np.float64).reshape(-1, 8)
    return Map(a[:, :3], a[:, 3], a[:, 4], a[:, 5], a[:, 6], a[:, 7])


# x, y, z, upper, lower, max_range, min_range, ratio -> the return it has to leave by from state (0, 0, 0), where T_sc = T_cs = I
WIDE = (4.0, -4.0, 16.0, 0.0, 1.0)
PLANTED = [
    ((0, 0, 1) + WIDE, OK),
    ((0, 0, 0.03125) + WIDE, DEPTH),
    ((0.125, 0.125, -1) + WIDE, DEPTH),              # behind the camera; u = 416, v = 192 would be inside
    ((-0.875, 0, 1) + WIDE, OK),                     # u == MinX
    ((-0.890625, 0, 1) + WIDE, U_LOW),               # u = 24
    ((1.0625, 0, 1) + WIDE, OK),                     # u == MaxX
    ((1.078125, 0, 1) + WIDE, U_HIGH),               # u = 1032
    ((0, -0.46875, 1) + WIDE, OK),                   # v == MinY
    ((0, -0.5, 1) + WIDE, V_LOW),                    # v = 0
    ((0, 0.5, 1) + WIDE, OK),                        # v == MaxY
    ((0, 0.53125, 1) + WIDE, V_HIGH),                # v = 528
    ((0, 0, 0.5) + WIDE, OK),                        # dist == min_dist
    ((0, 0, 0.25) + WIDE, DIST_LOW),
    ((0, 0, 8) + WIDE, OK),                          # dist == max_dist
    ((0, 0, 8.5) + WIDE, DIST_HIGH),
    ((0, 0, 2, 4.0, -4.0, 16.0, 2.0, 1.0), OK),      # dist == min_range
    ((0, 0, 2, 4.0, -4.0, 16.0, 2.5, 1.0), RANGE_LOW),
    ((0, 0, 4, 4.0, -4.0, 4.0, 0.0, 1.0), OK),       # dist == max_range
    ((0, 0, 4, 4.0, -4.0, 3.0, 0.0, 1.0), RANGE_HIGH),
    ((0, 0, 1, 0.0, 0.0, 16.0, 0.0, 1.0), OK),       # theta == lower == upper == 0 with delta x = 0
    ((0.25, 0, 1, 4.0, 1.0, 16.0, 0.0, 1.0), DIR_LOW),
    ((0.25, 0, 1, 0.125, -4.0, 16.0, 0.0, 1.0), DIR_HIGH),
]
HIDDEN = (0, 0, -1) + WIDE                            # a point no state at the origin sees
ORIGIN = np.zeros((1, 3), np.float32)


@functools.lru_cache(maxsize=None)
def planted_cases():
    """name -> Case, every one with the single state (0, 0, 0); the expected figures are asserted by tests/test_visibility_cpu.py"""
    vis = lambda ratio: (0, 0, 1, 4.0, -4.0, 16.0, 0.0, ratio)
    big_first = [vis(16777216.0)] + [HIDDEN] * 63 + [vis(1.0)] * 64
    return {
        "returns": Case(camera_exact(), _map_of([p for p, _ in PLANTED]), ORIGIN),
        # PcZ == 0.05f passes step 1; its dist is 0.05 too, so min_dist has to lie below it for the point to pass
        "depth_on": Case(camera_exact(min_dist=0.03125), _map_of([(0, 0, float(F(0.05))) + WIDE, (0, 0, 0.046875) + WIDE]), ORIGIN),
        "big_first": Case(camera_exact(), _map_of(big_first), ORIGIN),               # in point order the sum stays 16777216
        "big_last": Case(camera_exact(), _map_of(big_first[::-1]), ORIGIN),
        "half": Case(camera_exact(), _map_of([HIDDEN, vis(0.5)]), ORIGIN),           # 0.5 -> 1
        "two_and_half": Case(camera_exact(), _map_of([vis(1.0), HIDDEN, vis(1.0), vis(0.5)]), ORIGIN),   # 2.5 -> 3
    }


def golden_map():
    z = np.load(os.path.join(HERE, "golden", "planner_map_s.npz"))
    n = len(z["xyz"])
    return Map(z["xyz"], z["upper"], z["lower"], np.full(n, FLT_MAX, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32))


@functools.lru_cache(maxsize=None)
def golden_case(ns=300, seed=2681):
    """the reference's own planner map with the camera(map_data, int) constants; a state with a near pair is replaced by the next draw"""
    rng = np.random.default_rng(seed)
    cam, m = camera_with_map(), golden_map()
    states, replaced = draw_states(rng, ns), 0
    while True:
        bad = np.nonzero(near_pairs(cam, m, states).any(1))[0]
        if not len(bad):
            break
        states[bad] = draw_states(rng, len(bad))
        replaced += len(bad)
    return Case(cam, m, states, replaced=replaced)


def motions_of(case, sizes=(1, 2, 3, 40)):
    """consecutive runs of the case's states, one per size -> (list of state arrays, list of their count arrays)"""
    off = np.cumsum((0,) + tuple(sizes))
    return [case.states[a:b] for a, b in zip(off, off[1:])], [case.count[a:b] for a, b in zip(off, off[1:])]


def trajectories_of(case, thr):
    """-> name -> (indices into the case's states, expected index): the failing state first, in the middle (inside the first 64 states
    and past them) and absent (more than 64 states)"""
    good, bad = np.nonzero(case.count > thr)[0], np.nonzero(case.count <= thr)[0]
    assert len(good) >= 1 and len(bad) >= 1
    g = lambda k: list(np.resize(good, k))
    t = {"first": [bad[0]] + g(3), "middle": g(5) + [bad[0]] + g(3), "late": g(66) + [bad[-1]] + g(2), "absent": g(70), "one": g(1)}
    return {k: (np.array(v), advance_step(case.count[np.array(v)], thr)) for k, v in t.items()}
