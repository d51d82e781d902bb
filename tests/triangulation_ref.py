"""CPU restatement of the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:295-436) for the triangulation tests,
written from the reference's lines and the OpenCV conventions of DESIGN.md section 2.7.  It does not call the library.

float32 values are carried as Python floats that are exactly representable in float32; a float operation is the double operation
rounded once more (`f32`): for + - * / and sqrt of float32 operands the rounding through double is innocuous (53 >= 2 * 24 + 2
bits), so this IS the float operation.  Double expressions are plain Python arithmetic; sqrt / atan2 / cos are the C library's.

Also here: the seeded scene generator the CPU and GPU tests share, and the first-wins resolve over the neighbours of one keyframe."""
import math
import struct

import numpy as np

NO_MATCH, ACCEPTED, LOW_PARALLAX, W_ZERO, DEPTH1, DEPTH2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, SUPERSEDED = range(11)
BRANCH_NONE, BRANCH_SVD, BRANCH_STEREO1, BRANCH_STEREO2 = range(4)
FLT_EPSILON = 2.0 ** -23

OBS = np.dtype([("ux", "<f4"), ("uy", "<f4"), ("kx", "<f4"), ("ky", "<f4"), ("u_right", "<f4"), ("depth", "<f4"), ("octave", "<i4")])


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def ulps_apart(a, b):
    """distance of two float32 values in units of the last place of the larger one"""
    m = max(abs(a), abs(b))
    if m == 0:
        return 0.0
    return abs(a - b) / (2.0 ** (math.frexp(m)[1] - 24))


def scale_factors(n_levels=8, scale_factor=1.2):
    """mvScaleFactor[i] = mvScaleFactor[i - 1] * scaleFactor in float (src/ORBextractor.cc:416-421)"""
    sf = [1.0]
    for _ in range(1, n_levels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return np.array(sf, np.float32)


def keyframe(Tcw, fx, fy, cx, cy, mbf, sf):
    """the members of one keyframe the loop reads; mb = mbf / fx (src/Frame.cc:163)"""
    fx, fy, cx, cy, mbf = (f32(v) for v in (fx, fy, cx, cy, mbf))
    return dict(Tcw=np.asarray(Tcw, np.float32).reshape(4, 4), fx=fx, fy=fy, cx=cx, cy=cy, mbf=mbf, mb=f32(mbf / fx),
                scale_factors=np.asarray(sf, np.float32))


def _T(K):
    return [float(v) for v in np.asarray(K["Tcw"], np.float32).reshape(16)]


def _center(T):
    """Ow = -Rcw.t() * tcw (KeyFrame::SetPose): double accumulation in index order, one rounding"""
    return [f32(((T[k] * T[3] + T[4 + k] * T[7]) + T[8 + k] * T[11]) * -1.0) for k in range(3)]


def _rot_wc(T, v, add=(0.0, 0.0, 0.0)):
    """Rwc * v (+ addend widened to double): cv::Mat product"""
    return [f32(((T[i] * v[0] + T[4 + i] * v[1]) + T[8 + i] * v[2]) + add[i]) for i in range(3)]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cos_stereo(mb, depth):
    a = f32(math.atan2(f32(mb / 2), depth))
    return f32(math.cos(f32(2 * a)))


def jacobi_vt(A):
    """cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a float 4x4 (OpenCV 3.2 core/src/lapack.cpp, JacobiSVDImpl_<float>):
    -> (vt as 4 rows of float32 values, sweeps that rotated)"""
    At = [[f32(A[k][i]) for k in range(4)] for i in range(4)]
    V = [[1.0 if i == k else 0.0 for k in range(4)] for i in range(4)]
    W = [sum_sq(At[i]) for i in range(4)]
    eps = f32(FLT_EPSILON * 2)
    sweeps = 0
    for _ in range(30):
        changed = False
        for i in range(3):
            for j in range(i + 1, 4):
                Ai, Aj = At[i], At[j]
                a, b = W[i], W[j]
                p = 0.0
                for k in range(4):
                    p += Ai[k] * Aj[k]
                if abs(p) <= eps * math.sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = math.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = f32(math.sqrt(delta / gamma))
                    c = f32(p / (gamma * s * 2))
                else:
                    c = f32(math.sqrt((gamma + beta) / (gamma * 2)))
                    s = f32(p / (gamma * c * 2))
                a = b = 0.0
                for k in range(4):
                    t0 = f32(f32(c * Ai[k]) + f32(s * Aj[k]))
                    t1 = f32(f32(-s * Ai[k]) + f32(c * Aj[k]))
                    Ai[k], Aj[k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                Vi, Vj = V[i], V[j]
                for k in range(4):
                    t0 = f32(f32(c * Vi[k]) + f32(s * Vj[k]))
                    t1 = f32(f32(-s * Vi[k]) + f32(c * Vj[k]))
                    Vi[k], Vj[k] = t0, t1
        if not changed:
            break
        sweeps += 1
    W = [math.sqrt(sum_sq(At[i])) for i in range(4)]
    for i in range(3):
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            V[i], V[j] = V[j], V[i]
    return V, sweeps


def sum_sq(row):
    s = 0.0
    for v in row:
        s += v * v
    return s


def _reproj_ok(K, T, o, mbf, x3D, z):
    sf = float(K["scale_factors"][o["octave"]])
    sigma2 = f32(sf * sf)
    x = f32(_dot3(T[0:3], x3D) + T[3])
    y = f32(_dot3(T[4:7], x3D) + T[7])
    invz = f32(1.0 / z)
    u = f32(f32(f32(K["fx"] * x) * invz) + K["cx"])
    v = f32(f32(f32(K["fy"] * y) * invz) + K["cy"])
    ex, ey = f32(u - o["ux"]), f32(v - o["uy"])
    e2 = f32(f32(ex * ex) + f32(ey * ey))
    if not o["u_right"] >= 0:
        return not e2 > 5.991 * sigma2
    u_r = f32(u - f32(mbf * invz))
    er = f32(u_r - o["u_right"])
    return not f32(e2 + f32(er * er)) > 7.8 * sigma2


def triangulate_pair(K1, K2, o1, o2, info=None):
    """one matched pair -> (status, [x, y, z] float32 values); o1 / o2: records of OBS (or dicts with its fields).
    info (a dict) receives the branch, the Jacobi sweeps and the smallest distance in float ulps between the operands of a
    comparison that involves a cosParallaxStereo1 / 2 which came out of atan2 / cos."""
    o1 = {k: (int(o1[k]) if k == "octave" else float(o1[k])) for k in OBS.names}
    o2 = {k: (int(o2[k]) if k == "octave" else float(o2[k])) for k in OBS.names}
    T1, T2 = _T(K1), _T(K2)
    zero = [0.0, 0.0, 0.0]
    bStereo1, bStereo2 = o1["u_right"] >= 0, o2["u_right"] >= 0
    invfx1, invfy1, invfx2, invfy2 = f32(1.0 / K1["fx"]), f32(1.0 / K1["fy"]), f32(1.0 / K2["fx"]), f32(1.0 / K2["fy"])
    xn1 = [f32(f32(o1["ux"] - K1["cx"]) * invfx1), f32(f32(o1["uy"] - K1["cy"]) * invfy1), 1.0]
    xn2 = [f32(f32(o2["ux"] - K2["cx"]) * invfx2), f32(f32(o2["uy"] - K2["cy"]) * invfy2), 1.0]
    ray1, ray2 = _rot_wc(T1, xn1), _rot_wc(T2, xn2)
    cosRays = f32(_dot3(ray1, ray2) / (math.sqrt(_dot3(ray1, ray1)) * math.sqrt(_dot3(ray2, ray2))))
    cs1 = cs2 = f32(cosRays + 1)
    libm = False
    if bStereo1:
        cs1, libm = _cos_stereo(K1["mb"], o1["depth"]), True
    elif bStereo2:
        cs2, libm = _cos_stereo(K2["mb"], o2["depth"]), True
    cs = cs2 if cs2 < cs1 else cs1
    margin = min(ulps_apart(cs1, cs2), ulps_apart(cosRays, cs)) if libm else float("inf")
    branch = BRANCH_NONE
    if cosRays < cs and cosRays > 0 and (bStereo1 or bStereo2 or cosRays < 0.9998):
        branch = BRANCH_SVD
    elif bStereo1 and cs1 < cs2:
        branch = BRANCH_STEREO1 if o1["depth"] > 0 else BRANCH_NONE
    elif bStereo2 and cs2 < cs1:
        branch = BRANCH_STEREO2 if o2["depth"] > 0 else BRANCH_NONE
    if info is not None:
        info.update(branch=branch, margin_ulps=margin, sweeps=0)
    if branch == BRANCH_NONE:
        return LOW_PARALLAX, zero
    if branch == BRANCH_SVD:
        A = [[f32(f32(xn1[0] * T1[8 + k]) - T1[k]) for k in range(4)],
             [f32(f32(xn1[1] * T1[8 + k]) - T1[4 + k]) for k in range(4)],
             [f32(f32(xn2[0] * T2[8 + k]) - T2[k]) for k in range(4)],
             [f32(f32(xn2[1] * T2[8 + k]) - T2[4 + k]) for k in range(4)]]
        V, sweeps = jacobi_vt(A)
        if info is not None:
            info["sweeps"] = sweeps
        v = V[3]
        if v[3] == 0:
            return W_ZERO, zero
        r = f32(1.0 / v[3])
        x3D = [f32(v[k] * r) for k in range(3)]
    else:
        K, T, o = (K1, T1, o1) if branch == BRANCH_STEREO1 else (K2, T2, o2)
        z = o["depth"]
        invfx, invfy = f32(1.0 / K["fx"]), f32(1.0 / K["fy"])
        xc = [f32(f32(f32(o["kx"] - K["cx"]) * z) * invfx), f32(f32(f32(o["ky"] - K["cy"]) * z) * invfy), z]
        x3D = _rot_wc(T, xc, _center(T))
    z1 = f32(_dot3(T1[8:11], x3D) + T1[11])
    if z1 <= 0:
        return DEPTH1, x3D
    z2 = f32(_dot3(T2[8:11], x3D) + T2[11])
    if z2 <= 0:
        return DEPTH2, x3D
    if not _reproj_ok(K1, T1, o1, K1["mbf"], x3D, z1):
        return REPROJ1, x3D
    if not _reproj_ok(K2, T2, o2, K1["mbf"], x3D, z2):   # mpCurrentKeyFrame->mbf (:410)
        return REPROJ2, x3D
    Ow1, Ow2 = _center(T1), _center(T2)
    n1 = [f32(x3D[k] - Ow1[k]) for k in range(3)]
    n2 = [f32(x3D[k] - Ow2[k]) for k in range(3)]
    dist1, dist2 = f32(math.sqrt(_dot3(n1, n1))), f32(math.sqrt(_dot3(n2, n2)))
    if dist1 == 0 or dist2 == 0:
        return ZERO_DIST, x3D
    ratioDist = f32(dist2 / dist1)
    ratioOctave = f32(float(K1["scale_factors"][o1["octave"]]) / float(K2["scale_factors"][o2["octave"]]))
    ratioFactor = f32(1.5 * float(K1["scale_factors"][1]))
    if f32(ratioDist * ratioFactor) < ratioOctave or ratioDist > f32(ratioOctave * ratioFactor):
        return SCALE, x3D
    return ACCEPTED, x3D


def triangulate_matches(K1, K2, obs1, obs2, infos=None):
    """the matches of one (KF1, KF2) pair -> (status uint8 [n], x3D float32 [n][3])"""
    n = len(obs1)
    status, x3D = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    for k in range(n):
        info = {} if infos is not None else None
        status[k], x3D[k] = triangulate_pair(K1, K2, obs1[k], obs2[k], info)
        if infos is not None:
            infos.append(info)
    return status, x3D


def triangulate_frames(kfs1, obs_of1, n1, kfs2, obs_of2, n2, kf1, kf2, match12, first_wins, infos=None):
    """what aos2_frames_triangulate_matches computes: kfs* = keyframe() per frame of a batch, obs_of* = OBS arrays [batch][cap],
    n* = features per frame, match12 [n_pairs][cap] -> (status [n_pairs][cap], x3D [n_pairs][cap][3], nnew [n_pairs])"""
    P, cap = match12.shape
    status, x3D = np.zeros((P, cap), np.uint8), np.zeros((P, cap, 3), np.float32)
    for p in range(P):
        a, b = int(kf1[p]), int(kf2[p])
        for i in range(min(cap, int(n1[a]))):
            m = int(match12[p, i])
            if 0 <= m < int(n2[b]):
                info = {} if infos is not None else None
                status[p, i], x3D[p, i] = triangulate_pair(kfs1[a], kfs2[b], obs_of1[a][i], obs_of2[b][m], info)
                if infos is not None:
                    infos.append(info)
    if first_wins:
        resolve_first_wins(kf1, status)
    return status, x3D, (status == ACCEPTED).sum(1).astype(np.int32)


def resolve_first_wins(kf1, status):
    """the pairs that share kf1 are one CreateNewMapPoints call in call order: a feature's first accepted pair keeps it (the
    reference's next SearchForTriangulation skips a feature that holds a map point, src/ORBmatcher.cc:700-703)"""
    taken = {}
    for p in range(len(kf1)):
        t = taken.setdefault(int(kf1[p]), np.zeros(status.shape[1], bool))
        acc = status[p] == ACCEPTED
        status[p][acc & t] = SUPERSEDED
        t |= acc


# ------------------------------------------------------------------------------------------------------------- the generator
CAM_A = dict(fx=520.9, fy=521.0, cx=325.1, cy=249.7, mbf=80.0, w=640, h=480)
CAM_B = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, mbf=386.1448, w=1241, h=376)


def _small_pose(rng, shift):
    """Tcw of a camera rotated by a few degrees and displaced by `shift` (camera axes) from the origin"""
    w = rng.normal(0, 0.03, 3)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + math.sin(th) / th * Kx + (1 - math.cos(th)) / th ** 2 * Kx @ Kx
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.asarray(shift, float)   # camera centre at `shift`
    return T.astype(np.float32)


def scene(seed, n_feat=96, cams=(CAM_A, CAM_A, CAM_A, CAM_A), distort_keys=False):
    """Four frames that see the same n_feat world points: frame 0 at a small random pose near the origin, frames 1 and 2 displaced
    sideways by 0.25-0.5 m, frame 3 displaced 0.12 m along the optical axis (low ray parallax: the stereo fallbacks).  Depths
    log-uniform 0.5-60 m, octaves uniform 0-7, pixel noise 0.8 sigma x scale with 15 % of the observations at 12 x that; half the
    features of a frame are stereo where z < 40 mb, with 1 % depth noise.
    -> dict(kfs = keyframe() per frame, obs = OBS [4][n_feat], n = [4], sf)"""
    rng = np.random.default_rng(seed)
    sf = scale_factors()
    side = lambda: rng.uniform(0.25, 0.5) * rng.choice([-1.0, 1.0])   # noqa: E731
    shifts = [rng.normal(0, 0.02, 3), [side(), rng.normal(0, 0.03), rng.normal(0, 0.03)], [side(), rng.normal(0, 0.03), rng.normal(0, 0.03)],
              [rng.normal(0, 0.005), rng.normal(0, 0.005), 0.12]]
    Ts = [_small_pose(rng, s) for s in shifts]
    c0 = cams[0]
    z = np.exp(rng.uniform(math.log(0.5), math.log(60.0), n_feat))
    u = rng.uniform(40, c0["w"] - 40, n_feat)
    v = rng.uniform(40, c0["h"] - 40, n_feat)
    Pc = np.stack([(u - c0["cx"]) / c0["fx"] * z, (v - c0["cy"]) / c0["fy"] * z, z, np.ones(n_feat)])
    Pw = np.linalg.inv(Ts[0].astype(float)) @ Pc
    kfs, obs = [], np.zeros((4, n_feat), OBS)
    for f in range(4):
        c = cams[f]
        kfs.append(keyframe(Ts[f], c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], sf))
        pc = Ts[f].astype(float) @ Pw
        octave = rng.integers(0, 8, n_feat)
        sigma = 0.8 * sf[octave] * np.where(rng.random(n_feat) < 0.15, 12.0, 1.0)
        zc = np.where(np.abs(pc[2]) < 1e-3, 1e-3, pc[2])
        ux = c["fx"] * pc[0] / zc + c["cx"] + rng.normal(0, 1, n_feat) * sigma
        uy = c["fy"] * pc[1] / zc + c["cy"] + rng.normal(0, 1, n_feat) * sigma
        stereo = (rng.random(n_feat) < 0.5) & (pc[2] > 0) & (pc[2] < 40 * kfs[f]["mb"])
        depth = np.where(stereo, pc[2] * (1 + 0.01 * rng.normal(0, 1, n_feat)), -1.0).astype(np.float32)
        o = obs[f]
        o["ux"], o["uy"] = ux.astype(np.float32), uy.astype(np.float32)
        o["kx"], o["ky"] = o["ux"], o["uy"]
        if distort_keys:   # mvKeys != mvKeysUn, as with a distorted camera: UnprojectStereo must read mvKeys
            o["kx"] += rng.normal(0, 1.5, n_feat).astype(np.float32)
            o["ky"] += rng.normal(0, 1.5, n_feat).astype(np.float32)
        o["depth"] = depth
        with np.errstate(divide="ignore"):
            o["u_right"] = np.where(stereo, o["ux"] - np.float32(kfs[f]["mbf"]) / depth, np.float32(-1.0)).astype(np.float32)
        o["octave"] = octave
    return dict(kfs=kfs, obs=obs, n=np.full(4, n_feat, np.int32), sf=sf, seed=seed)


def matches(seed, n_feat, pairs, frac=0.7, wrong=0.2):
    """match12 [len(pairs)][n_feat]: 70 % of a keyframe's features are matched -- to the same world point, 20 % of them to a wrong one"""
    rng = np.random.default_rng(1000 + seed)
    m = np.full((len(pairs), n_feat), -1, np.int32)
    for p in range(len(pairs)):
        on = rng.random(n_feat) < frac
        bad = on & (rng.random(n_feat) < wrong)
        partner = np.arange(n_feat)
        partner[bad] = (partner[bad] + rng.integers(1, n_feat, bad.sum())) % n_feat
        m[p, on] = partner[on]
    return m


PAIRS6 = ((0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3))   # 2 keyframes x 3 neighbours, neighbour order = call order
CAMS = {"same": (CAM_A, CAM_A, CAM_A, CAM_A), "mixed": (CAM_A, CAM_B, CAM_A, CAM_B)}
_cases = {}


def generator_case(seed, cams="same", distort_keys=False):
    """the scene of `seed`, the matches of PAIRS6 and the reference's results on them, computed once per process and shared by the
    tests (read-only): dict(scene, kf1, kf2, match12, infos, status / nnew (first_wins), status_all / nnew_all (without), x3D)"""
    key = (seed, cams, distort_keys)
    if key not in _cases:
        S = scene(seed, cams=CAMS[cams], distort_keys=distort_keys)
        kf1 = np.array([p[0] for p in PAIRS6], np.int32)
        kf2 = np.array([p[1] for p in PAIRS6], np.int32)
        m = matches(seed, S["obs"].shape[1], PAIRS6)
        infos = []
        st_all, x3D, nnew_all = triangulate_frames(S["kfs"], S["obs"], S["n"], S["kfs"], S["obs"], S["n"], kf1, kf2, m, False, infos)
        st = st_all.copy()
        resolve_first_wins(kf1, st)
        c = dict(scene=S, kf1=kf1, kf2=kf2, match12=m, infos=infos, status=st, nnew=(st == ACCEPTED).sum(1).astype(np.int32),
                 status_all=st_all, nnew_all=nnew_all, x3D=x3D)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[key] = c
    return _cases[key]
