"""One edge pass and one outlier pass of Optimizer::PoseOptimization, written from the g2o operation in numpy long double with a scale M >= |q|
for every quantity q -- the reference of tests/test_pose_pass_gpu.py (the tap aos2_debug_pose_pass_device: `pass` and the reclassification of
pose_optimization_body alone, in each of its instantiations) -- two float64 models of the same pass that set the tolerance, and the inputs.

The operation (g2o: types_six_dof_expmap.cpp:266-364, base_unary_edge.hpp, robust_kernel_impl.cpp:78-91; Optimizer.cc:239-452), from a pose
(qx qy qz qw tx ty tz, double), the float32 map points, observations and weights, and the edges' level / robust flags:
    p = R X + t;  e = obs - cam_project(p)
        mono: (fx x / z + cx, fy y / z + cy);  stereo: invz = (float)(1 / z), (x invz fx + cx, y invz fy + cy, x invz fx + cx - bf invz)
        (the float reciprocal is part of the operation; bf is a double member of the pose-only stereo edge, so bf invz -- two float32
        values -- is an exact double product, unlike the float product of the two-vertex edge in lba_system_ref)
    chi2_e = w e.e;  Huber with delta = (float)sqrt(5.991) mono, (float)sqrt(7.815) stereo where the edge is robust:
        rho = chi2, rho' = 1 within delta^2;  rho = 2 sqrt(chi2) delta - delta^2, rho' = delta / sqrt(chi2) beyond
    J: linearizeOplus of the two pose-only edges, with invz = 1 / z, invz_2 = invz invz as written there
    H = sum J^T (rho' w) J,  b = -sum J^T rho' w e,  chi2 = sum rho      over the edges at level 0
    outlier pass: chi2_e of an edge flagged outlier is recomputed at the pose, another edge keeps its stored value;
        outlier = level1 = (float)chi2_e > 7.815f (stereo) / 5.991f (mono);  robust cleared in round 2;  nBad = the number of outliers
Values, scales (VM: value, m, f) and omega = |q_dev - q_ref| / (2^-53 M_q), M = m + f, are those of tests/lba_system_ref.py.
"""
import numpy as np

import lba_system_ref as S
from lba_system_ref import DELTA, LD, U53, VM

MARGIN = 4.0                                                   # as tests/test_lba_system_gpu.py
FORMS = ((4, 256), (8, 256), (9, 128), (0, 256))               # form -> (kEpt, NT) of pose_optimization_body
FORM_MAX = (1024, 2048, 1152, None)
QUANTITIES = ("H_diag", "H_off", "b", "chi2", "chi2_edge")
IU = np.triu_indices(6)                                        # the 21 entries of H, row by row
DIAG = np.array([0, 6, 11, 15, 18, 20])
OFF = np.array([k for k in range(21) if k not in (0, 6, 11, 15, 18, 20)])
THRESH = (np.float32(5.991), np.float32(7.815))
SLOT_SIZES = {0: (3, 33, 63, 64, 65, 255, 256, 257, 300, 511, 513, 767, 769, 1023, 1024),
              1: (3, 257, 1025, 1279, 1280, 1281, 1535, 1537, 2047, 2048),
              2: (3, 127, 128, 129, 255, 257, 1023, 1024, 1025, 1151, 1152),
              3: (3, 257, 1025, 2049, 2500)}
MUTATIONS = ("rt_block", "one_entry", "jac_f32", "b_alt", "no_huber_H", "no_row3", "invz_mono", "level1_chi2")


def seq_sum(a):
    """the sum over axis 0 in index order (numpy's own sum is pairwise)"""
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1:], a.dtype)


def flags(case, name, default):
    v = case.get(name)
    return np.full(case["n"], default, np.uint8) if v is None else np.asarray(v, np.uint8)


def inputs(case, dt):
    n = case["n"]
    X = np.asarray(case["Xw"], np.float32).reshape(n, 3).astype(dt)
    obs = np.asarray(case["obs"], np.float32).reshape(n, 3)
    st = np.asarray(case["stereo"]).astype(np.uint8)
    w = np.asarray(case["inv_sigma2"], np.float32).astype(dt)
    pose = np.asarray(case["pose"], np.float64).astype(dt)
    return n, X, obs, st, w, pose


# ------------------------------------------------------------------------------------------ the operation
def camera_points(case, dt):
    n, X, _, _, _, pose = inputs(case, dt)
    Rm = S.rot_from_quat(pose[None, :4])[0]
    col = lambda v: VM(np.full(n, v, dt))
    return [col(Rm[r, 0]) * VM(X[:, 0]) + col(Rm[r, 1]) * VM(X[:, 1]) + col(Rm[r, 2]) * VM(X[:, 2]) + col(pose[4 + r]) for r in range(3)]


def residual(case, p, dt, exact_reciprocal=False, float_invz_on_mono=False):
    """computeError of both pose-only edges -> (list of 3 VM, third zero for a mono edge; 1 / z of the arithmetic)"""
    n, _, obs, st, _, _ = inputs(case, dt)
    fx, fy, cx, cy, bf = S.cam(case, dt)
    x, y, z = p
    um, vm_ = x / z * fx + cx, y / z * fy + cy
    rz = 1 / z.v
    if exact_reciprocal:
        invz = 1 / z
        bfz = invz * bf
    else:   # const float invz = 1.0f / trans_xyz[2]: one rounding of the quotient to float; exact from there
        iv = rz.astype(np.float32).astype(dt)
        invz = VM(iv)
        bfz = VM(bf * iv)
    us, vs = x * invz * fx + cx, y * invz * fy + cy
    stb = st.astype(bool)
    sel = lambda m, a, b: VM(*(np.where(m, getattr(a, k), getattr(b, k)) for k in ("v", "m", "f")))
    zero = VM(np.zeros(n, dt))
    o = [VM(obs[:, i].astype(dt)) for i in range(3)]
    fl = stb | float_invz_on_mono
    return [o[0] - sel(fl, us, um), o[1] - sel(fl, vs, vm_), sel(stb, o[2] - (us - bfz), zero)], rz


def jacobian(case, p, dt):
    """linearizeOplus of EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose -> [3][6] VM (third row zero: mono)"""
    n, _, _, st, _, _ = inputs(case, dt)
    fx, fy, cx, cy, bf = S.cam(case, dt)
    x, y, z = p
    invz = 1 / z
    invz_2 = invz * invz
    zero = VM(np.zeros(n, dt))
    s = st.astype(dt)
    J0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
    J1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
    J2 = [(J0[0] - bf * y * invz_2) * s, (J0[1] + bf * x * invz_2) * s, J0[2] * s, J0[3] * s, zero, (J0[5] - bf * invz_2) * s]
    return [J0, J1, J2]


def edge_pass(case, dt=LD):
    """-> dict: sums (28: H upper triangle, b, robust chi2) and chi2_edge [n] as (value, M) pairs, edges summed in insertion order;
    active, beyond (of all edges, as if active), depth, rz = 1 / z"""
    n, _, _, st, w, _ = inputs(case, dt)
    active = ~flags(case, "level1", 0).astype(bool)
    robust = flags(case, "robust", 1).astype(bool)
    p = camera_points(case, dt)
    e, rz = residual(case, p, dt)
    w = VM(w)
    chi2 = (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) * w
    delta = np.where(st == 1, DELTA[1], DELTA[0]).astype(dt)
    beyond = robust & (chi2.v > delta * delta)
    sq = np.sqrt(np.where(beyond, chi2.v, 1))
    one = np.ones_like(sq)
    rel = np.where(beyond, chi2.f / np.where(beyond, chi2.v, 1), 0) / 2 + 1   # (a relative error of chi2 is half that of its root)
    rho = VM(*(np.where(beyond, a, b) for a, b in ((2 * sq * delta - delta * delta, chi2.v), (2 * np.sqrt(chi2.m) * delta + delta * delta, chi2.m),
                                                    (2 * sq * delta * (rel + 1) + np.abs(2 * sq * delta - delta * delta), chi2.f))))
    rho1 = VM(np.where(beyond, delta / sq, one), np.where(beyond, delta / sq, one), np.where(beyond, delta / sq * (rel + 1), 0 * one))
    W = rho1 * w
    J = jacobian(case, p, dt)
    act = active.astype(dt)
    terms = [(J[0][r] * W * J[0][c] + J[1][r] * W * J[1][c] + J[2][r] * W * J[2][c]) * act for r, c in zip(*IU)]
    terms += [-(J[0][r] * W * e[0] + J[1][r] * W * e[1] + J[2][r] * W * e[2]) * act for r in range(6)]
    terms.append(rho * act)
    v = np.array([seq_sum(t.v) for t in terms])
    M = np.array([(t.m + t.f).sum() for t in terms])
    return dict(sums=(v, M), chi2_edge=(chi2.v, chi2.m + chi2.f), active=active, beyond=beyond, depth=p[2].v, rz=rz, J=J, e=e, dt=dt)


def case_key(case):
    """cases made from one problem share its arrays: the arrays' identity, the pose and the flags name a computation"""
    return (id(case["Xw"]), id(case["obs"]), id(case["inv_sigma2"]), np.asarray(case["pose"], np.float64).tobytes(), flags(case, "level1", 0).tobytes(),
            flags(case, "robust", 1).tobytes())


def reference(case):
    key = ("ref",) + case_key(case)
    if key not in _cache:
        _cache[key] = (edge_pass(case, LD), case)   # (the case is kept: its arrays' ids stay theirs)
    return _cache[key][0]


def model_textbook(case):
    """float64 model (a): the operation as written, every operation in float64, edges in insertion order"""
    r = edge_pass(case, np.float64)
    return dict(sums=r["sums"][0], chi2_edge=r["chi2_edge"][0])


def model_kernel(case, form, mutate=None):
    """float64 model (b), the kernel's form: the rotation as a matrix applied innermost-first, one reciprocal iz = 1 / z, a = x iz, b = y iz,
    the Jacobian from a, b, iz; a thread (tid = e mod NT) adds its edges in slot order, row by row; the 64 threads of a wave are added
    l + (l + 32), then l + (l + 16), then a binary tree over the 16; the waves in order.  mutate: one of MUTATIONS, a wrong assembly."""
    f8 = np.float64
    n, X, obs, st, w, pose = inputs(case, f8)
    fx, fy, cx, cy, bf = S.cam(case, f8)
    NT = FORMS[form][1]
    active = ~flags(case, "level1", 0).astype(bool)
    robust = flags(case, "robust", 1).astype(bool)
    R = S.rot_from_quat(pose[None, :4])[0]
    x, y, z = (R[r, 2] * X[:, 2] + (R[r, 1] * X[:, 1] + (R[r, 0] * X[:, 0] + pose[4 + r])) for r in range(3))
    iz = 1.0 / z
    a, b = x * iz, y * iz
    izf = iz.astype(np.float32).astype(f8)
    s0, s1 = x * izf * fx + cx, y * izf * fy + cy
    s2 = s0 - bf * izf
    stb = st.astype(bool)
    fl = stb | (mutate == "invz_mono")
    ob = obs.astype(f8)
    e0, e1, e2 = ob[:, 0] - np.where(fl, s0, a * fx + cx), ob[:, 1] - np.where(fl, s1, b * fy + cy), np.where(stb, ob[:, 2] - s2, 0.0)
    c = e0 * (w * e0) + e1 * (w * e1) + e2 * (w * e2)
    delta = np.where(stb, DELTA[1], DELTA[0])
    dsqr = delta * delta
    hub = robust & (c > dsqr)
    sq = np.sqrt(np.where(hub, c, 1.0))
    cr = np.where(hub, 2 * sq * delta - dsqr, c)
    r1 = np.where(hub, delta / sq, 1.0)
    wo = np.where(hub, r1 * w, w)
    fxz, fyz, ab = fx * iz, fy * iz, a * b
    zero = np.zeros(n)
    bfz2 = bf * (iz * iz)
    J = [ab * fx, -((a * a + 1.0) * fx), b * fx, -fxz, zero, a * fxz,
         (b * b + 1.0) * fy, -(ab * fy), -(a * fy), zero, -fyz, b * fyz]
    J += [-bfz2 * y + J[0], bfz2 * x + J[1], J[2], J[3], zero, J[5] - bfz2]
    if mutate == "jac_f32":
        J = [j.astype(np.float32).astype(f8) for j in J]
    woH = w if mutate == "no_huber_H" else wo
    wo2 = np.where(stb, woH, 0.0) if mutate != "no_row3" else zero
    we = [r1 * (w * e0), r1 * (w * e1), np.where(stb, r1 * (w * e2), 0.0)]
    rows = np.zeros((3, n, 28))   # the three fused multiply-adds of an entry, in the kernel's order
    for m, (r, c2) in enumerate(zip(*IU)):
        rows[0, :, m], rows[1, :, m], rows[2, :, m] = (J[r] * woH) * J[c2], (J[6 + r] * woH) * J[6 + c2], (J[12 + r] * wo2) * J[12 + c2]
    for r in range(6):
        rows[0, :, 21 + r], rows[1, :, 21 + r], rows[2, :, 21 + r] = -J[r] * we[0], -J[6 + r] * we[1], -J[12 + r] * we[2]
    rows[0, :, 27] = cr
    rows *= active[None, :, None]
    if mutate == "level1_chi2":
        rows[0, ~active, 27] = c[~active]
    nsl = (n + NT - 1) // NT
    pad = np.zeros((3, nsl * NT, 28))
    pad[:, :n] = rows
    pad = pad.reshape(3, nsl, NT, 28)
    acc = np.zeros((NT, 28))
    for j in range(nsl):
        acc[:, 27] += pad[0, j, :, 27]   # (the robust chi2 goes first)
        for k in range(3):
            acc[:, :27] += pad[k, j, :, :27]
    fin = np.zeros(28)
    for wv in range(NT // 64):
        v = acc[64 * wv:64 * wv + 64]
        v = v[:32] + v[32:]
        v = v[:16] + v[16:]
        while len(v) > 1:
            v = v[0::2] + v[1::2]
        fin = v[0] if wv == 0 else fin + v[0]
    if mutate == "rt_block":
        H = np.zeros((6, 6))
        H[IU] = fin[:21]
        H[:3, 3:] *= 0.99
        fin[:21] = H[IU]
    if mutate == "one_entry":
        fin[10] *= 0.9   # H(1, 5)
    if mutate == "b_alt":
        fin[21:27] *= 1 + 1e-3 * np.array([1, -1, 1, -1, 1, -1])
    return dict(sums=fin, chi2_edge=c)


def chi2_quat_f64(case):
    """float64 model of po_edge_error + edge_chi2: Eigen's quaternion * vector, the divisions of project2d"""
    f8 = np.float64
    n, X, obs, st, w, pose = inputs(case, f8)
    fx, fy, cx, cy, bf = S.cam(case, f8)
    q, t = pose[:4], pose[4:]
    uv = 2 * np.cross(q[:3], X)
    p = X + q[3] * uv + np.cross(q[:3], uv) + t
    ob = obs.astype(f8)
    izf = (1.0 / p[:, 2]).astype(np.float32).astype(f8)
    s0, s1 = p[:, 0] * izf * fx + cx, p[:, 1] * izf * fy + cy
    stb = st.astype(bool)
    e0 = ob[:, 0] - np.where(stb, s0, p[:, 0] / p[:, 2] * fx + cx)
    e1 = ob[:, 1] - np.where(stb, s1, p[:, 1] / p[:, 2] * fy + cy)
    e2 = np.where(stb, ob[:, 2] - (s0 - bf * izf), 0.0)
    return e0 * (w * e0) + e1 * (w * e1) + e2 * (w * e2)


# ------------------------------------------------------------------------------------------ the measure
def omega(g, v, M):
    g, v, M = np.asarray(g, LD), np.asarray(v, LD), np.asarray(M, LD)
    d = np.abs(g - v)
    return np.where(d == 0, LD(0), d / (U53 * np.where(M > 0, M, LD("1e-4000")))).astype(np.float64)


def omegas(ref, got, edges=None):
    """got: dict with sums [28] and / or chi2_edge [n] (compared on `edges`, default the active ones) -> dict quantity -> worst omega"""
    out = {}
    if "sums" in got:
        om = omega(got["sums"], *ref["sums"])
        out.update(H_diag=om[DIAG].max(), H_off=om[OFF].max(), b=om[21:27].max(), chi2=om[27])
    if "chi2_edge" in got:
        sel = ref["active"] if edges is None else edges
        out["chi2_edge"] = omega(np.asarray(got["chi2_edge"])[sel], ref["chi2_edge"][0][sel], ref["chi2_edge"][1][sel]).max() if sel.any() else 0.0
    return {k: float(v) for k, v in out.items()}


def model_omegas(case):
    """-> (dict quantity -> worst omega of the two float64 models, dict model -> its omegas)"""
    key = ("models", case["form"]) + case_key(case)
    if key not in _cache:
        ref = reference(case)
        per = dict(textbook=omegas(ref, model_textbook(case)), kernel=omegas(ref, model_kernel(case, case["form"])))
        _cache[key] = ({q: max(per[m][q] for m in per) for q in QUANTITIES}, per)
    return _cache[key]


def family_tolerance(cases_):
    """the omega the device has to meet per quantity: MARGIN x the worst omega of the two float64 models over the family"""
    tol = {q: 0.0 for q in QUANTITIES}
    for c in cases_:
        for q, v in model_omegas(c)[0].items():
            tol[q] = max(tol[q], v)
    return {q: MARGIN * v for q, v in tol.items()}


def recomputed_tolerance(form):
    """the omega the chi2 that the outlier pass recomputes has to meet: MARGIN x the worst omega of its two float64 models -- the
    quaternion-rotate form of po_edge_error and the matrix form -- over the frames of the form's outlier family, all edges"""
    key = ("recomputed", form)
    if key not in _cache:
        worst = 0.0
        for case in cases("slots", form):
            ref = reference(case)
            every = np.ones(case["n"], bool)
            for got in (chi2_quat_f64(case), model_kernel(case, form)["chi2_edge"]):
                worst = max(worst, omegas(ref, dict(chi2_edge=got), every)["chi2_edge"])
        _cache[key] = MARGIN * worst
    return _cache[key]


def near_float_boundary(case):
    """stereo edges whose long-double 1 / z lies within 2^-48 relative of a float32 rounding boundary (the midpoint of two neighbours)"""
    ref = reference(case)
    r = ref["rz"]
    f = r.astype(np.float32)
    with np.errstate(over="ignore"):
        mids = [(f.astype(LD) + np.nextafter(f, np.float32(s) * np.float32(np.inf)).astype(LD)) / 2 for s in (-1, 1)]
    d = np.minimum(np.abs(r - mids[0]), np.abs(r - mids[1])) / np.abs(r)
    return (d < LD(2.0) ** -48) & np.asarray(case["stereo"]).astype(bool)


def outlier_reference(case, tol_edge):
    """the outlier pass of round case["it"] from the long-double chi2 -> dict: chi2 (value, M), recomputed, outlier, robust, left_out (edges
    whose decision changes when chi2_ref moves by +- its allowance tol_edge 2^-53 M), n_bad over the other edges"""
    ref = reference(dict(case, level1=None, robust=None))   # (chi2_e does not depend on the flags: one reference for the four rounds)
    n = case["n"]
    st = np.asarray(case["stereo"]).astype(bool)
    rec = flags(case, "outlier", 0).astype(bool)
    stored = np.asarray(case["chi2"], np.float64).astype(LD)
    chi = np.where(rec, ref["chi2_edge"][0], stored)
    M = np.where(rec, ref["chi2_edge"][1], np.abs(stored))
    thr = np.where(st, THRESH[1], THRESH[0])
    dec = lambda v: v.astype(np.float32) > thr
    allow = np.where(rec, LD(tol_edge) * U53 * M, 0)
    out = dec(chi)
    left = (dec(chi - allow) != out) | (dec(chi + allow) != out)
    rb = flags(case, "robust", 1) * (0 if case["it"] == 2 else 1)
    return dict(chi2=(chi, M), recomputed=rec, outlier=out.astype(np.uint8), robust=rb.astype(np.uint8), left_out=left, n_bad=int(out[~left].sum()), n=n)


# ------------------------------------------------------------------------------------------ the inputs
_cache = {}


def synth():
    import __graft_entry__ as graft
    return graft.load_package().synth


def problem(seed, n, i, **kw):
    """synth_pose_problem with mono-only, stereo-only and mixed edges and the two cameras cycling as in test_pose_optimization_slot_count_boundaries,
    a start pose 0.003 rad / 0.015 away (20-50 % of the edges beyond the Huber delta), and the pose as 7 doubles"""
    s = synth()
    kw = dict(dict(stereo_frac=(0.0, 1.0, 0.6)[i % 3], cfg=("tum", "kitti")[i % 2], rot_err=0.003, trans_err=0.015), **kw)
    p = s.synth_pose_problem(seed, n=n, **kw)
    p["pose"] = s.tcw_to_qt(p["Tcw"])
    return p


def rot(rv):
    return S.rotvec_to_R(np.asarray(rv, np.float64))


def geometry_problem(seed, n, kind):
    """hand-built frames: 'depth' 0.5 .. 50 (log-uniform), 'far_pose' |t| up to 10 and a rotation near pi, 'levels' weights of all eight
    pyramid levels in equal shares, 'behind' a fifth of the points behind the camera (z < 0: PoseOptimization's edges do not reject them)"""
    s = synth()
    rng = np.random.default_rng(seed)
    c = s.CONFIGS["kitti"]
    fx, fy, cx, cy, bf = (float(np.float32(c[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
    if kind == "far_pose":
        ax = rng.normal(size=3)
        Rcw, tcw = rot(ax / np.linalg.norm(ax) * (np.pi - 0.02)), rng.uniform(-1, 1, 3) * np.array([10.0, 6.0, 9.5])
        tcw[0] = 10.0 * np.sign(tcw[0])
    else:
        Rcw, tcw = rot(rng.uniform(-0.2, 0.2, 3)), rng.uniform(-1, 1, 3)
    z = 10 ** rng.uniform(np.log10(0.55), np.log10(48.0), n) if kind == "depth" else rng.uniform(3.0, 40.0, n)
    if kind == "behind":
        z[::5] *= -1
    u, v = rng.uniform(20, c["w"] - 20, n), rng.uniform(20, c["h"] - 20, n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = ((Xc - tcw) @ Rcw).astype(np.float32)
    lvl = np.arange(n) % 8 if kind == "levels" else np.minimum(rng.geometric(0.4, n) - 1, 7)
    sf = np.float32(1.2) ** lvl.astype(np.float32)
    sig = sf.astype(np.float64)
    stereo = rng.random(n) < 0.6
    du, dv, dr = (rng.normal(0, 1, n) * sig for _ in range(3))
    obs = np.stack([u + du, v + dv, np.where(stereo, u + du - bf / np.abs(z) + dr, -1.0)], 1).astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = rot(rng.normal(0, 0.003 / np.sqrt(3), 3)) @ Rcw
    T[:3, 3] = tcw + rng.normal(0, 0.015 / np.sqrt(3), 3)
    T = T.astype(np.float32)
    return dict(n=n, Xw=Xw, obs=obs, stereo=stereo.astype(np.uint8), inv_sigma2=(np.float32(1.0) / (sf * sf)).astype(np.float32),
                fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, Tcw=T.reshape(16), pose=s.tcw_to_qt(T.reshape(16)))


# seeds of the slot-boundary frames that replace 9000 + 100 form + i: at those the start pose leaves under 20 % of the edges on one side of
# the Huber delta for the reference (test_pose_pass_cpu.py asserts the shares of every frame)
SEEDS = {(1, 1025): 10102, (2, 1023): 13206, (2, 1024): 10207}
LEVEL1_PATTERNS = ("scatter", "wave", "slot", "all_but_three")
ROBUST_PATTERNS = ("on", "off", "mixed")
GEOMETRY = ("depth", "far_pose", "levels", "behind")


def flags_n(form):
    return 300 if form == 2 else 700   # three slots of every form, the last partly filled, several waves


def level1_pattern(name, base, form, rng):
    n, NT = base["n"], FORMS[form][1]
    e = np.arange(n)
    if name == "scatter":
        return (rng.random(n) < 0.3).astype(np.uint8)
    if name == "wave":
        return ((e % NT) // 64 == 1).astype(np.uint8)
    if name == "slot":
        return (e // NT == 1).astype(np.uint8)
    beyond = reference(dict(base, form=form))["beyond"]   # three edges stay, on both sides of the Huber delta
    keep = [int(np.nonzero(~beyond)[0][5]), int(np.nonzero(beyond)[0][3]), int(np.nonzero(~beyond)[0][-2])]
    l1 = np.ones(n, np.uint8)
    l1[keep] = 0
    return l1


def replaced(case, seed=77):
    """the case with other data in its level-1 edges: another finite point, another observation, a weight up to 1e6"""
    rng = np.random.default_rng(seed)
    l1 = case["level1"].astype(bool)
    k = int(l1.sum())
    Xw, obs, w = (np.array(case[x], np.float32) for x in ("Xw", "obs", "inv_sigma2"))
    Xw[l1] = rng.uniform(-50, 50, (k, 3)).astype(np.float32)
    obs[l1] = rng.uniform(-2000, 2000, (k, 3)).astype(np.float32)
    w[l1] = (10 ** rng.uniform(-2, 6, k)).astype(np.float32)
    return dict(case, Xw=Xw, obs=obs, inv_sigma2=w, name=case["name"] + " replaced")


def cases(family, form):
    """-> list of case dicts (a problem with name, family, form, pose and the flags / round / stored chi2 the tap takes)"""
    key = (family, form)
    if key in _cache:
        return _cache[key]
    mk = lambda name, p, **kw: dict(p, name=name, family=family, form=form, **kw)
    if family == "slots":
        out = [mk("n%d" % n, problem(SEEDS.get((form, n), 9000 + 100 * form + i), n, i)) for i, n in enumerate(SLOT_SIZES[form])]
    elif family == "flags":
        base = problem(9500 + form, flags_n(form), 2)
        rng = np.random.default_rng(40 + form)
        out = []
        for lp in LEVEL1_PATTERNS:
            l1 = level1_pattern(lp, base, form, rng)
            for rp in ROBUST_PATTERNS:
                rb = dict(on=np.ones(base["n"], np.uint8), off=np.zeros(base["n"], np.uint8), mixed=(rng.random(base["n"]) < 0.5).astype(np.uint8))[rp]
                out.append(mk("%s/%s" % (lp, rp), base, level1=l1, robust=rb))
    elif family == "geometry":
        out = [mk(k, geometry_problem(9700 + 10 * form + i, 600, k)) for i, k in enumerate(GEOMETRY)]
    elif family == "outlier":
        out = []
        for b in cases("slots", form):
            n = b["n"]
            rng = np.random.default_rng(9800 + n)
            stored = model_textbook(b)["chi2_edge"]
            for it in range(4):
                ou = np.zeros(n, np.uint8)
                ou[rng.permutation(n)[:max(1, n // 3)]] = 1   # a scattered third
                chi = np.where(ou == 1, 1e9, stored)   # (stale values where the pass has to recompute)
                out.append(dict(b, name="%s it%d" % (b["name"], it), family=family, it=it, outlier=ou, level1=ou.copy(),
                                robust=np.full(n, 1 if it < 3 else 0, np.uint8), chi2=chi))
    elif family == "whole":
        ns = SLOT_SIZES[form] + (2, 9)
        out = [mk("n%d" % n, problem(9900 + 100 * form + i, n, i, outlier_frac=(0.05, 0.3)[i % 2], rot_err=0.01, trans_err=0.05)) for i, n in enumerate(ns)]
    else:
        raise KeyError(family)
    _cache[key] = out
    return out


PASS_FAMILIES = [(f, form) for form in range(4) for f in ("slots", "flags")] + [("geometry", 0), ("geometry", 3)]
