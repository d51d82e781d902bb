"""TEST INFRASTRUCTURE: the planner's motion checks -- StateValidChecker::GetShortestPath / twb_shortpath / twb_gettangent /
twb_getangle (src/StateValidChecker.cc:313-518), myprop (:296-311), the state loop of checkMotionTW / reconstructMotionTW / MotionCost
(:244-294, :543-578), MotionCostLength / MotionCostCamera (:522-541), isValid (:97-119) and collisionDetection::check_collisions
(src/collisions.cc:70-94) -- restated literally in Python floats (IEEE doubles, no FMA), with tw_sin / tw_cos / tw_atan2 as the same
operation sequences csrc/motion_tw.h writes down.  The counts come from tests/visibility_ref.py.  Also here: the scene of the golden
planner map and obstacles, the seeded draw of motions and the planted cases, shared by the CPU and the GPU tests."""
import functools
import math
import os

import numpy as np

import visibility_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
INF, NAN = float("inf"), float("nan")
PI = 3.1416                      # include/StateValidChecker.h:26
MAX_SEGMENT_STATES = 1 << 20     # AOS2_SVC_MAX_SEGMENT_STATES


# ---------------------------------------------------------------------------------------- IEEE where Python raises
def div(a, b):
    if b == 0.0:
        if a == 0.0 or a != a:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def sqrt(x):
    return NAN if x < 0.0 else math.sqrt(x)


# ---------------------------------------------------------------------------------------- math (csrc/motion_tw.h)
def tw_reduce(x):
    v = x * 6.36619772367581382433e-01 + 0.5
    if v != v or abs(v) >= 4503599627370496.0:
        return x - x, 0.0, 0
    fk = float(math.floor(v))
    t = x - fk * 1.57079632673412561417e+00
    w = fk * 6.07710050650619224932e-11
    r = t - w
    y = (t - r) - w
    return r, y, int(fk - 4.0 * math.floor(fk * 0.25))


def kernel_sin(x, y):
    z = x * x
    v = z * x
    r = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (
        -2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))
    return x - ((z * (0.5 * y - v * r) - y) - v * -1.66666666666666324348e-01)


def kernel_cos(x, y):
    z = x * x
    w = z * z
    r = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) + \
        (w * w) * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))
    hz = 0.5 * z
    w = 1.0 - hz
    return w + (((1.0 - w) - hz) + (z * r - x * y))


def tw_sin(x):
    r, y, q = tw_reduce(x)
    return (kernel_sin(r, y), kernel_cos(r, y), -kernel_sin(r, y), -kernel_cos(r, y))[q]


def tw_cos(x):
    r, y, q = tw_reduce(x)
    return (kernel_cos(r, y), -kernel_sin(r, y), -kernel_cos(r, y), kernel_sin(r, y))[q]


def atan_pos(x):
    if x != x:
        return x
    if x >= 2.0 ** 66:
        return 1.57079632679489655800e+00 + 6.12323399573676603587e-17
    if x < 0.4375:
        if x < 2.0 ** -29:
            return x
        idx, hi, lo = -1, 0.0, 0.0
    elif x < 1.1875:
        if x < 0.6875:
            idx, hi, lo = 0, 4.63647609000806093515e-01, 2.26987774529616870924e-17
            x = (2.0 * x - 1.0) / (2.0 + x)
        else:
            idx, hi, lo = 1, 7.85398163397448278999e-01, 3.06161699786838301793e-17
            x = (x - 1.0) / (x + 1.0)
    elif x < 2.4375:
        idx, hi, lo = 2, 9.82793723247329054082e-01, 1.39033110312309984516e-17
        x = (x - 1.5) / (1.0 + 1.5 * x)
    else:
        idx, hi, lo = 3, 1.57079632679489655800e+00, 6.12323399573676603587e-17
        x = -1.0 / x
    z = x * x
    w = z * z
    s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 + w * (
        6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))))
    s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 + w * (
        -5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))))
    if idx < 0:
        return x - x * (s1 + s2)
    return hi - ((x * (s1 + s2) - lo) - x)


def tw_atan2(y, x):
    pi, pi_lo = 3.1415926535897931160e+00, 1.2246467991473531772e-16
    if x != x or y != y:
        return x + y
    yneg, xneg = math.copysign(1.0, y) < 0, math.copysign(1.0, x) < 0
    if y == 0.0:
        return ((-pi if yneg else pi) if xneg else y)
    if x == 0.0:
        return -1.5707963267948965580e+00 if yneg else 1.5707963267948965580e+00
    z = atan_pos(abs(div(y, x)))
    if not xneg:
        return -z if yneg else z
    return (z - pi_lo) - pi if yneg else pi - (z - pi_lo)


# ---------------------------------------------------------------------------------------- the reference's functions
class Params:
    """aos2_svc_params_t with the reference's constants (include/StateValidChecker.h:28-31, include/collisions.h:30-33)"""

    def __init__(self, **kw):
        self.turn_radius, self.robot_r, self.dt = 0.25, 0.4, 0.3
        self.min_x, self.max_x, self.min_y, self.max_y = -1.15, 6.5, -5.0, 5.0
        self.max_dist_heuristic, self.start, self.heuristic, self.feature_threshold = 2.0, (0.0, 0.0, 0.0), 0, -1
        for k, v in kw.items():
            assert hasattr(self, k)
            setattr(self, k, v)

    def to_capi(self, pkg):
        p = pkg.SvcParams()
        for k in ("turn_radius", "robot_r", "dt", "min_x", "max_x", "min_y", "max_y", "max_dist_heuristic"):
            setattr(p, k, float(getattr(self, k)))
        for i in range(3):
            p.start[i] = float(self.start[i])
        p.heuristic, p.feature_threshold = int(self.heuristic), int(self.feature_threshold)
        return p


def norm_distance(a1, a2, d):
    s = 0.0
    for i in range(d):
        s += (a1[i] - a2[i]) * (a1[i] - a2[i])
    return sqrt(s)


def getangle(q1, q2):
    return tw_atan2(q2[1] - q1[1], q2[0] - q1[0])


def gettangent(q1, s1, q2, s2, turn_radius):
    """:420-512 -> qt1, qt2"""
    if s1 == s2:
        ux = q2[0] - q1[0]
        uy = q2[1] - q1[1]
        norm_u = sqrt(ux * ux + uy * uy)
        if s1 == 1:
            return ([q1[0] + div(turn_radius * uy, norm_u), q1[1] - div(turn_radius * ux, norm_u)],
                    [q2[0] + div(turn_radius * uy, norm_u), q2[1] - div(turn_radius * ux, norm_u)])
        return ([q1[0] - div(turn_radius * uy, norm_u), q1[1] + div(turn_radius * ux, norm_u)],
                [q2[0] - div(turn_radius * uy, norm_u), q2[1] + div(turn_radius * ux, norm_u)])
    qmid_x = (q2[0] - q1[0]) / 2
    qmid_y = (q2[1] - q1[1]) / 2
    L = sqrt(qmid_x * qmid_x + qmid_y * qmid_y)
    x = div(turn_radius * turn_radius, L)
    y = div(turn_radius, L) * sqrt((L * L) - (turn_radius * turn_radius))
    qmid_x = div(qmid_x, L)
    qmid_y = div(qmid_y, L)
    if s1 == 1:
        return ([q1[0] + x * qmid_x + y * qmid_y, q1[1] + x * qmid_y - y * qmid_x],
                [q2[0] - x * qmid_x - y * qmid_y, q2[1] - x * qmid_y + y * qmid_x])
    return ([q1[0] + x * qmid_x - y * qmid_y, q1[1] + x * qmid_y + y * qmid_x],
            [q2[0] - x * qmid_x + y * qmid_y, q2[1] - x * qmid_y - y * qmid_x])


def shortpath(q1, s1, q2, s2, dr, turn_radius):
    """:370-418 -> d1mid2, or None where the reference returns valid = false"""
    h1, h2 = q1[2], q2[2]
    qc1 = [q1[0] - turn_radius * s1 * tw_sin(h1), q1[1] + turn_radius * s1 * tw_cos(h1)]
    qc2 = [q2[0] - turn_radius * s2 * tw_sin(h2), q2[1] + turn_radius * s2 * tw_cos(h2)]
    if s1 * s2 < 0 and norm_distance(qc1, qc2, 2) < 2 * turn_radius:
        return None
    qt1, qt2 = gettangent(qc1, dr * s1, qc2, dr * s2, turn_radius)
    delta1 = getangle(qc1, qt1) - getangle(qc1, q1)
    if dr * s1 > 0 and delta1 < 0:
        delta1 += 2 * PI
    elif dr * s1 < 0 and delta1 > 0:
        delta1 -= 2 * PI
    delta2 = getangle(qc2, q2) - getangle(qc2, qt2)
    if dr * s2 > 0 and delta2 < 0:
        delta2 += 2 * PI
    elif dr * s2 < 0 and delta2 > 0:
        delta2 -= 2 * PI
    return [abs(turn_radius * delta1), norm_distance(qt1, qt2, 2), abs(turn_radius * delta2)]


CANDIDATES = [(s1, s2, dr) for s1 in (-1, 1) for s2 in (-1, 1) for dr in (-1, 1)]   # the loops :337-339


def candidates(q1, q2, turn_radius):
    """d1mid2 (or None) of the eight candidates, in order"""
    return [shortpath(q1, s1, q2, s2, dr, turn_radius) for s1, s2, dr in CANDIDATES]


def myprop(q, vi, wi, ti):
    h = q[2] + wi * ti
    if wi:
        x = q[0] + (div(vi, wi) * (tw_sin(h) - tw_sin(q[2])))
        y = q[1] - (div(vi, wi) * (tw_cos(h) - tw_cos(q[2])))
    else:
        x = q[0] + ti * vi * tw_cos(h)
        y = q[1] + ti * vi * tw_sin(h)
    return [x, y, h]


class TooLong(Exception):
    pass


class Path:
    """GetShortestPath (:313-367) and reconstructMotionTW (:273-294)"""

    def __init__(self, q1, q2, p):
        q1, q2 = [float(v) for v in q1], [float(v) for v in q2]
        d, best = [1e9, 1e9, 1e9], -1
        for k, t in enumerate(candidates(q1, q2, p.turn_radius)):
            if t is not None:
                if t[0] + t[1] + t[2] < d[0] + d[1] + d[2]:
                    best, d = k, list(t)
        self.valid, self.type = best >= 0, best
        self.t, self.m, self.Q = [0.0] * 3, [0] * 3, [q1]
        if best < 0:
            return
        s1, s2, dr = CANDIDATES[best]
        self.t = d
        v = [dr, dr, dr]
        w = [s1 * v[0] / p.turn_radius, 0.0, s2 * v[2] / p.turn_radius]
        for i in range(3):
            md = 1 + math.ceil(d[i] / p.dt)
            if md > MAX_SEGMENT_STATES + 1:
                raise TooLong()
            m = int(md)
            self.m[i] = m
            dd = div(d[i], float(m - 1))
            q = self.Q[-1]
            for j in range(1, m):
                self.Q.append(myprop(q, float(v[i]), w[i], j * dd))


class Scene:
    """a StateValidChecker: camera and map, obstacles, parameters -- with the restatement's answers"""

    def __init__(self, cam, vmap, obstacles, obs_r=0.1, params=None):
        self.cam, self.map = cam, vmap
        self.obs = np.ascontiguousarray(obstacles, np.float64).reshape(-1, 2)
        self.obs_r, self.p = float(obs_r), params or Params()
        self.rows = vmap.rows()
        self._counts = {}

    @property
    def thr(self):
        return self.cam.feature_threshold if self.p.feature_threshold == -1 else self.p.feature_threshold

    def count(self, q):
        """countVisible of the state narrowed to float (src/camera.cc:249 -> :135)"""
        f = (R.F(q[0]), R.F(q[1]), R.F(q[2]))
        key = np.array(f, np.float32).tobytes()
        if key not in self._counts:
            self._counts[key] = R.count_visible(self.cam, self.rows, R.state_from_xyt(f[0], f[1], f[2], self.cam), self.map.n)[0]
        return self._counts[key]

    def nearest2(self, q):
        """min over the obstacles of (0 + dx*dx) + dy*dy: elementwise IEEE doubles, so the same bits as a scalar loop"""
        with np.errstate(all="ignore"):
            dx, dy = q[0] - self.obs[:, 0], q[1] - self.obs[:, 1]
            return float(((0.0 + dx * dx) + dy * dy).min())

    def collision_free(self, q):
        """check_collisions(q, robot_r) src/collisions.cc:70-94"""
        p = self.p
        if len(self.obs) == 0:
            return True
        if q[0] < p.min_x or q[1] > p.max_x or q[2] < p.min_y or q[2] > p.max_y:
            return False
        return not (sqrt(self.nearest2(q)) <= p.robot_r + self.obs_r)

    def is_valid(self, q):
        """isValid (:97-119)"""
        p = self.p
        if not self.collision_free(q):
            return False
        if not p.heuristic:
            return self.count(q) > self.thr
        if (q[0] - p.start[0]) * (q[0] - p.start[0]) + (q[1] - p.start[1]) * (q[1] - p.start[1]) < p.max_dist_heuristic * p.max_dist_heuristic:
            return self.count(q) > self.thr
        return True

    def valid(self, states):
        """-> what capi.StateValidChecker.valid returns"""
        st = np.asarray(states, np.float64).reshape(-1, 3)
        return dict(valid=np.array([self.is_valid(q) for q in st], np.uint8).reshape(-1),
                    collision_free=np.array([self.collision_free(q) for q in st], np.uint8).reshape(-1),
                    count=np.array([self.count(q) for q in st], np.int32).reshape(-1))

    def motion(self, q1, q2):
        P = Path(q1, q2, self.p)
        Q, first, length, camera = P.Q, -1, 0.0, 0.0
        for i in range(1, len(Q)):
            if first < 0 and not self.is_valid(Q[i]):     # checkMotionTW :264
                first = i
            length += norm_distance(Q[i - 1], Q[i], 3)    # MotionCostLength :526
            if i < len(Q) - 1:                            # MotionCostCamera :534-539
                c = self.count(Q[i])
                camera += div(1., 1e-4) if c < self.thr else div(1., float(c))
        return dict(path_valid=int(P.valid), type=P.type, t=P.t, m=P.m, n_states=len(Q), valid=int(P.valid and first < 0),
                    first_invalid=first, cost_length=length, cost_camera=camera, Q=Q)

    def motions(self, q1, q2):
        """-> what capi.StateValidChecker.motions returns (with states)"""
        res = [self.motion(a, b) for a, b in zip(np.asarray(q1, np.float64).reshape(-1, 3), np.asarray(q2, np.float64).reshape(-1, 3))]
        n = len(res)
        out = dict(path_valid=np.array([r["path_valid"] for r in res], np.uint8).reshape(n),
                   type=np.array([r["type"] for r in res], np.int32).reshape(n),
                   t=np.array([r["t"] for r in res], np.float64).reshape(n, 3), m=np.array([r["m"] for r in res], np.int32).reshape(n, 3),
                   n_states=np.array([r["n_states"] for r in res], np.int32).reshape(n),
                   valid=np.array([r["valid"] for r in res], np.uint8).reshape(n),
                   first_invalid=np.array([r["first_invalid"] for r in res], np.int32).reshape(n),
                   cost_length=np.array([r["cost_length"] for r in res], np.float64).reshape(n),
                   cost_camera=np.array([r["cost_camera"] for r in res], np.float64).reshape(n))
        out["offsets"] = np.cumsum([0] + [r["n_states"] for r in res]).astype(np.int32)
        out["states"] = np.array([q for r in res for q in r["Q"]], np.float64).reshape(-1, 3)
        return out

    def load(self, pkg, device=0):
        S = pkg.StateValidChecker(device=device)
        S.vis.set_camera(self.cam.to_capi(pkg))
        S.vis.set_map(*self.map.args())
        S.set_obstacles(self.obs, self.obs_r)
        S.set_params(self.p.to_capi(pkg))
        return S


FIELDS = ("path_valid", "type", "t", "m", "n_states", "valid", "first_invalid", "cost_length", "cost_camera", "offsets", "states")


def same(got, want, sel=None):
    """every output bit for bit; sel: the motions of `want` that `got` holds, in order (a prefix count or None for all)"""
    if sel is not None:
        k = sel
        n = int(want["offsets"][k])
        want = {f: (want[f][:k + 1] if f == "offsets" else want[f][:n] if f == "states" else want[f][:k]) for f in FIELDS}
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        assert got[f].tobytes() == want[f].tobytes(), f


# ---------------------------------------------------------------------------------------- the golden scene and the draw
def golden_obstacles():
    z = np.load(os.path.join(HERE, "golden", "planner_obstacles.npz"))
    return z["xy"], z["r"]


@functools.lru_cache(maxsize=None)
def golden_scene():
    """the reference's planner map and its data/obs.txt; obs_r is the class default 0.1 (include/collisions.h:61): the FloorMap
    constructor never reads the file's r column"""
    case = R.golden_case()
    return Scene(case.cam, case.map, golden_obstacles()[0], 0.1)


@functools.lru_cache(maxsize=None)
def golden_starts():
    """the states of visibility_ref.golden_case() that are valid: count > 20 and collision free"""
    case, S = R.golden_case(), golden_scene()
    keep = [i for i in range(len(case.states)) if case.count[i] > 20 and S.collision_free([float(v) for v in case.states[i]])]
    return case.states[keep].astype(np.float64)


def draw_motion(rng, starts):
    """q1 one of the starts; q2 0.2-1.2 m ahead within +-0.6 rad of the heading, its heading changed by +-0.5 rad"""
    q1 = starts[rng.integers(len(starts))]
    d, a = rng.uniform(0.2, 1.2), q1[2] + rng.uniform(-0.6, 0.6)
    return q1, np.array([q1[0] + d * math.cos(a), q1[1] + d * math.sin(a), q1[2] + rng.uniform(-0.5, 0.5)])


class Draw:
    pass


@functools.lru_cache(maxsize=None)
def golden_draw(nm=90, seed=11):
    """nm motions on the golden scene with the restatement's answers.  A motion with a state whose visibility count sits on a
    rounding boundary (visibility_ref.near_pairs) is replaced by the next draw."""
    rng, S, starts = np.random.default_rng(seed), golden_scene(), golden_starts()
    q1, q2, replaced = [], [], 0
    while len(q1) < nm:
        a, b = draw_motion(rng, starts)
        Q = np.array(Path(a, b, S.p).Q, np.float64)
        if R.near_pairs(S.cam, S.map, Q.astype(np.float32)).any():
            replaced += 1
            continue
        q1.append(a)
        q2.append(b)
    D = Draw()
    D.scene, D.q1, D.q2, D.replaced = S, np.array(q1), np.array(q2), replaced
    D.want = S.motions(D.q1, D.q2)
    return D


def outcome(D):
    """per motion: 'valid', 'collision' (the first invalid state fails check_collisions) or 'visibility'"""
    w, out = D.want, []
    for k in range(len(D.q1)):
        if w["valid"][k]:
            out.append("valid")
        else:
            q = w["states"][w["offsets"][k] + w["first_invalid"][k]]
            out.append("visibility" if D.scene.collision_free(q) else "collision")
    return out


# ---------------------------------------------------------------------------------------- the sweep scene and the planted cases
SWEEP_SEED = 5


@functools.lru_cache(maxsize=None)
def sweep_draw(nm=300, seed=23):
    """nm motions from the golden starts over the golden obstacles, with a map of 130 random points (visibility_ref.random_case)
    under the exact camera: cheap to restate, so this is the draw the shape sweeps use.  The threshold is the median count of the
    states, so both sides of it occur."""
    case = R.random_case(SWEEP_SEED, 130)
    rng, starts = np.random.default_rng(seed), golden_starts()
    probe = Scene(case.cam, case.map, golden_obstacles()[0], 0.1)
    q1, q2, replaced, counts = [], [], 0, []
    while len(q1) < nm:
        a, b = draw_motion(rng, starts)
        Q = np.array(Path(a, b, probe.p).Q, np.float64)
        if R.near_pairs(case.cam, case.map, Q.astype(np.float32)).any():
            replaced += 1
            continue
        q1.append(a)
        q2.append(b)
        counts += [probe.count(q) for q in Q]
    D = Draw()
    D.scene = Scene(case.cam, case.map, golden_obstacles()[0], 0.1, Params(feature_threshold=int(np.median(counts))))
    D.scene._counts = probe._counts
    D.q1, D.q2, D.replaced = np.array(q1), np.array(q2), replaced
    D.want = D.scene.motions(D.q1, D.q2)
    return D


def with_obstacles(D, n, k=64):
    """the first k motions of a draw against the n obstacles nearest to their states -> (scene, want)"""
    S0 = D.scene
    st = D.want["states"][: D.want["offsets"][k]]
    d = np.min((st[:, None, 0] - S0.obs[None, :, 0]) ** 2 + (st[:, None, 1] - S0.obs[None, :, 1]) ** 2, 0)
    S = Scene(S0.cam, S0.map, S0.obs[np.argsort(d, kind="stable")[:n]], S0.obs_r, S0.p)
    S._counts = S0._counts
    return S, S.motions(D.q1[:k], D.q2[:k])


def with_map(D, vmap, k=64):
    S0 = D.scene
    S = Scene(S0.cam, vmap, S0.obs, S0.obs_r, S0.p)
    return S, S.motions(D.q1[:k], D.q2[:k])


def empty_map():
    z = np.zeros(0, np.float32)
    return R.Map(np.zeros((0, 3), np.float32), z, z, z, z, z)


@functools.lru_cache(maxsize=None)
def planted_types(seed=3):
    """type -> (q1, q2): the first motion of a seeded search that each of the eight candidates wins (goals on every side of q1)"""
    rng, p, found = np.random.default_rng(seed), Params(), {}
    while len(found) < 8:
        q1 = np.array([rng.uniform(0, 3), rng.uniform(-2, 2), rng.uniform(-3, 3)])
        q2 = q1 + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-2, 2)])
        P = Path(q1, q2, p)
        if P.valid and P.type not in found:
            found[P.type] = (q1, q2)
    return found


HALF_PI = 1.5707963267948966
PLANTED_MOTIONS = {
    "tie": ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)),                # straight ahead: t0 = t2 = 0, candidates 1 and 7 have the same total
    "same": ((1.0, 1.0, 0.5), (1.0, 1.0, 0.5)),               # q1 == q2
    "close": ((0.0, 0.0, 0.0), (0.0, 0.1, 3.0)),              # the opposite-turn circles 0.1 apart: four candidates infeasible
    "none": ((0.0, 0.0, 0.0), (4e9, 0.0, 0.0)),               # every total is 3e9 or more: no candidate wins
    "heading5": ((1.0, 1.0, 4.8), (1.0 + 0.6 * math.cos(5.0), 1.0 + 0.6 * math.sin(5.0), 5.4)),
    "y65": ((0.0, 6.3, HALF_PI), (0.0, 6.9, HALF_PI)),
}


@functools.lru_cache(maxsize=None)
def planted_scene():
    """the planted motions and one motion per winning type over the sweep's map, with three obstacles far from all of them (so that
    the bounds test runs and the nearest-obstacle query never rejects)"""
    case = R.random_case(SWEEP_SEED, 130)
    names = list(PLANTED_MOTIONS) + ["type%d" % t for t in range(8)]
    pairs = [PLANTED_MOTIONS[k] for k in PLANTED_MOTIONS] + [planted_types()[t] for t in range(8)]
    D = Draw()
    D.names = names
    D.q1, D.q2 = np.array([a for a, _ in pairs], np.float64), np.array([b for _, b in pairs], np.float64)
    D.scene = Scene(case.cam, case.map, [[100.0, 100.0], [-100.0, 50.0], [30.0, -100.0]], 0.1, Params(feature_threshold=-2))   # count > -2: visibility rejects nothing here
    D.want = D.scene.motions(D.q1, D.q2)
    D.replaced = 0
    return D


@functools.lru_cache(maxsize=None)
def planted_states():
    """states of visibility_ref.random_case inside the bounds, and obstacles planted against them -> a Draw with .states, .scene and
    the indices .on (an obstacle EXACTLY robot_r + obs_r away), .off (one a hair further), .eq (count == threshold)"""
    case = R.random_case(SWEEP_SEED, 130)
    st = case.states.astype(np.float64)
    keep = np.nonzero((st[:, 0] > -1.0) & (np.abs(st[:, 2]) < 3.0))[0][:40]
    st, cnt = st[keep], case.count[keep]
    thr = int(np.sort(cnt)[len(cnt) // 2])
    D = Draw()
    D.states = st
    D.eq = int(np.nonzero(cnt == thr)[0][0])
    hi, lo = np.nonzero(cnt > thr)[0], np.nonzero(cnt <= thr)[0]
    D.on, D.off, near = int(hi[0]), int(hi[1]), int([i for i in lo if i != D.eq][0])
    obs = [[st[D.on][0] + 0.5, st[D.on][1]],                            # dx = -0.5 exactly: sqrt(0.25) <= 0.4 + 0.1 rejects
           [st[D.off][0] + 0.5000000001, st[D.off][1]],
           [st[near][0] + 0.125, st[near][1] - 0.25]]
    D.scene = Scene(case.cam, case.map, obs, 0.1, Params(feature_threshold=thr))
    D.want = D.scene.valid(st)
    return D


def heuristic_scene():
    """the planted states with heuristicValidityCheck on: beyond max_dist_heuristic of the start, the count is not asked for"""
    D = planted_states()
    S = D.scene
    H = Scene(S.cam, S.map, S.obs, S.obs_r, Params(feature_threshold=S.thr, heuristic=1, start=tuple(D.states[D.eq]), max_dist_heuristic=2.0))
    H._counts = S._counts
    return H


def math_samples():
    x = np.linspace(-40.0, 40.0, 100000)
    g = np.concatenate([-np.logspace(-3, 3, 150)[::-1], np.logspace(-3, 3, 150)])          # 300 values of both signs
    Y, X = np.meshgrid(g, g)
    axes = [(0.0, v) for v in g] + [(v, 0.0) for v in g] + [(-0.0, v) for v in g] + [(v, -0.0) for v in g] + \
           [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    ay = np.concatenate([Y.ravel(), [a for a, _ in axes]])
    ax = np.concatenate([X.ravel(), [b for _, b in axes]])
    return x, ay, ax
