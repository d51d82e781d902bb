"""The linear system of one Levenberg-Marquardt trial of LocalBundleAdjustment, written from the g2o operation in numpy long double,
with a scale M >= |q| for every entry q -- the reference of tests/test_lba_system_gpu.py (the tap aos2_debug_lba_assemble_device:
k_lin, k_lm_init, k_schur alone) -- two float64 models of the same assembly that set the tolerance, and the hand-built windows.

The operation (g2o: types_six_dof_expmap.{h,cpp}, base_binary_edge.hpp, robust_kernel_impl.cpp, block_solver.hpp;
Optimizer.cc:507-660), from the double estimates (qx qy qz qw tx ty tz per keyframe, X per landmark) and the edges' level / robust flags:
    p = R X + t;  e = obs - proj(p)   (mono: plain; stereo: cam_project's float reciprocal invz = (float)(1 / z) and float bf * invz)
    chi2 = w e.e;  Huber with delta = (float)sqrt(5.991) mono, (float)sqrt(7.815) stereo when the edge is robust:
        rho = chi2, rho' = 1 within delta^2, rho = 2 sqrt(chi2) delta - delta^2, rho' = delta / sqrt(chi2) beyond
    J_l, J_pose: linearizeOplus, with the divisions as written there
    Hll_l = sum J_l^T (rho' w) J_l,  b_l = -sum J_l^T rho' w e,  Hpp_i, b_i alike,  B_il = J_pose^T (rho' w) J_l  (6 x 3)
    lambda_init = 1e-5 max |diag|,  chi2 = sum rho
    Hs_ij = [i = j] (Hpp_i + lambda I) - sum_l B_il (Hll_l + lambda I)^-1 B_jl^T,  bs_i = b_i - sum_l B_il (Hll_l + lambda I)^-1 b_l
Edges of fixed keyframes enter Hll and b_l only, masked (level 1) edges nothing.

The scale.  Every quantity is carried as (value, m, f).  m is the same expression with every term replaced by its absolute value --
inside p (|R||X| + |t|) and inside each Jacobian entry; what is divided by enters with its value -- and D^-1 replaced by
|D^-1| + |D^-1| M_D |D^-1|, M_D = M_Hll + lambda I (the conditioning of nearly rank-2 landmark blocks).  m alone misses the
conditioning of a depth or a chi2 that is formed with cancellation and then divided by (the float64 models reach omega = 4000 on Hll
with it), so f carries the first-order bound of what float64 leaves in the value, in units of 2^-53: the rounding of every operation
plus what the operands' errors become (a +- b: f_a + f_b + |v|; a b: |a| f_b + f_a |b| + |v|; a / b: f_a / |b| + |v| f_b / |b| + |v|).
M = m + f >= |q|, and omega = |q_dev - q_ref| / (2^-53 M_q).
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
DELTA = (float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))))   # mono, stereo
QUANTITIES = ("Hll", "b_l", "Hpp", "b_p", "Hs_diag", "Hs_off", "bs", "lambda", "chi2")


# ------------------------------------------------------------------------------------------ values with scales
class VM:
    """arrays of values v with m, the same expression in absolute values (what is divided by enters with its value), and f, the
    first-order bound of the error that float64 arithmetic leaves in v, in units of 2^-53: the rounding of every operation and what
    the operands' errors become (inputs are exact).  The arithmetic is the arrays' (long double: the reference, float64: model (a))."""
    __slots__ = ("v", "m", "f")
    __array_ufunc__ = None   # (numpy scalars and arrays on the left defer to the reflected operators)

    def __init__(self, v, m=None, f=None):
        self.v = v
        self.m = np.abs(v) if m is None else m
        self.f = np.zeros_like(v) if f is None else f

    def __add__(self, o):
        o = vm(o, self.v.dtype)
        v = self.v + o.v
        return VM(v, self.m + o.m, self.f + o.f + np.abs(v))

    def __sub__(self, o):
        o = vm(o, self.v.dtype)
        v = self.v - o.v
        return VM(v, self.m + o.m, self.f + o.f + np.abs(v))

    def __rsub__(self, o):
        return vm(o, self.v.dtype) - self

    def __mul__(self, o):
        o = vm(o, self.v.dtype)
        v = self.v * o.v
        return VM(v, self.m * o.m, np.abs(self.v) * o.f + self.f * np.abs(o.v) + np.abs(v))

    __radd__, __rmul__ = __add__, __mul__

    def __neg__(self):
        return VM(-self.v, self.m, self.f)

    def __truediv__(self, o):
        o = vm(o, self.v.dtype)
        v = self.v / o.v
        return VM(v, self.m / np.abs(o.v), self.f / np.abs(o.v) + np.abs(v) * o.f / np.abs(o.v) + np.abs(v))

    def __rtruediv__(self, o):
        return vm(o, self.v.dtype) / self


def vm(x, dt):
    return x if isinstance(x, VM) else VM(np.asarray(x, dt))


def stack(rows):
    """nested lists of VM -> (v, m, f) arrays [E, ...]"""
    return tuple(np.moveaxis(np.array([[getattr(c, k) for c in r] for r in rows]), -1, 0) for k in ("v", "m", "f"))


# ------------------------------------------------------------------------------------------ the operation
def rot_from_quat(q):
    """Eigen's Quaternion::toRotationMatrix, [n, 4] (x y z w) -> [n, 3, 3]"""
    x, y, z, w = (q[:, i] for i in range(4))
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])
    return np.moveaxis(R, -1, 0)


def cam(win, dt):
    return tuple(dt(float(np.float32(win[k]))) for k in ("fx", "fy", "cx", "cy", "bf"))


def residual(win, p, obs, stereo, dt, exact_reciprocal=False):
    """computeError of both edge kinds from camera points p (list of 3 VM) -> list of 3 VM (third: zero for a mono edge)"""
    fx, fy, cx, cy, bf = cam(win, dt)
    x, y, z = p
    um, vm_ = x / z * fx + cx, y / z * fy + cy
    if exact_reciprocal:
        invz = 1 / z
        bfz = invz * bf
    else:   # const float invz = 1.0f / trans_xyz[2];  res[2] = res[0] - bf * invz  (bf: const float &)
        iv = (1 / z.v.astype(np.float64)).astype(np.float32)
        invz = VM(iv.astype(dt))   # (the float reciprocal and the float product are the operation's: exact)
        bfz = VM((np.float32(win["bf"]) * iv).astype(dt))
    us, vs = x * invz * fx + cx, y * invz * fy + cy
    st = stereo.astype(bool)
    sel = lambda a, b: VM(*(np.where(st, getattr(a, k), getattr(b, k)) for k in ("v", "m", "f")))
    zero = VM(np.zeros_like(x.v))
    o = [VM(obs[:, i].astype(dt)) for i in range(3)]
    return [o[0] - sel(us, um), o[1] - sel(vs, vm_), sel(o[2] - (us - bfz), zero)]


def jacobians(win, R, p, stereo, dt):
    """linearizeOplus of EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ -> J_l [3][3], J_pose [3][6] (lists of VM; third rows zero: mono)"""
    fx, fy, cx, cy, bf = cam(win, dt)
    x, y, z = p
    z_2 = z * z
    st = stereo.astype(dt)
    zero = VM(np.zeros_like(x.v))
    Jl = [[-fx * R[0][c] / z + fx * x * R[2][c] / z_2 for c in range(3)], [-fy * R[1][c] / z + fy * y * R[2][c] / z_2 for c in range(3)]]
    Jl.append([(Jl[0][c] - bf * R[2][c] / z_2) * st for c in range(3)])
    Jp = [[x * y / z_2 * fx, -(1 + (x * x / z_2)) * fx, y / z * fx, -1 / z * fx, zero, x / z_2 * fx],
          [(1 + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy, zero, -1 / z * fy, y / z_2 * fy]]
    Jp.append([(Jp[0][0] - bf * y / z_2) * st, (Jp[0][1] + bf * x / z_2) * st, Jp[0][2] * st, Jp[0][3] * st, zero, (Jp[0][5] - bf / z_2) * st])
    return Jl, Jp


def camera_points(win, est, dt):
    pose, point = est["pose"].astype(dt), est["point"].astype(dt)
    ep, el = win["edge_pose"], win["edge_point"]
    Rm = rot_from_quat(pose[:, :4])[ep]
    R = [[VM(Rm[:, r, c]) for c in range(3)] for r in range(3)]
    X = [VM(point[el, i]) for i in range(3)]
    t = [VM(pose[ep, 4 + i]) for i in range(3)]
    p = [R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r] for r in range(3)]
    return R, p


def index_maps(win):
    """buildIndexMapping: free keyframes / landmarks with an edge, by id -> hpose, hpoint"""
    fixed = np.asarray(win["pose_fixed"]).astype(bool)
    used_p = np.zeros(win["n_poses"], bool)
    used_p[win["edge_pose"]] = True
    used_l = np.zeros(win["n_points"], bool)
    used_l[win["edge_point"]] = True
    hp = np.nonzero(used_p & ~fixed)[0]
    hl = np.nonzero(used_l)[0]
    hp = hp[np.argsort(np.asarray(win["pose_id"])[hp], kind="stable")]
    hl = hl[np.argsort(np.asarray(win["point_id"])[hl], kind="stable")]
    return hp.astype(np.int32), hl.astype(np.int32)


def mat3_inverse(D):
    """[n, 3, 3] by cofactors, in D's arithmetic"""
    a, b, c, d, e, f, g, h, i = (D[:, r, k] for r in range(3) for k in range(3))
    A, B, C_ = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * B + c * C_
    adj = np.array([[A, -(b * i - c * h), b * f - c * e], [B, a * i - c * g, -(a * f - c * d)], [C_, -(a * h - b * g), a * e - b * d]])
    return np.moveaxis(adj, -1, 0) / det[:, None, None]


def linearise(win, est, dt=LD):
    """the per-edge part and the block sums that do not depend on lambda -> dict of (value, scale) pairs and the index structure"""
    E = win["n_edges"]
    ep, el = np.asarray(win["edge_pose"]), np.asarray(win["edge_point"])
    stereo = np.asarray(win["edge_stereo"]).astype(np.uint8)
    active = ~np.asarray(est["e_level1"]).astype(bool)
    robust = np.asarray(est["e_robust"]).astype(bool)
    hp, hl = index_maps(win)
    n_p, n_l = len(hp), len(hl)
    ph = np.full(win["n_poses"], -1)
    ph[hp] = np.arange(n_p)
    lh = np.full(win["n_points"], -1)
    lh[hl] = np.arange(n_l)
    R, p = camera_points(win, est, dt)
    e = residual(win, p, np.asarray(win["edge_obs"], np.float32), stereo, dt)
    w = VM(np.asarray(win["edge_inv_sigma2"], np.float32).astype(dt))
    chi2 = (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) * w
    delta = np.where(stereo == 1, DELTA[1], DELTA[0]).astype(dt)
    beyond = robust & (chi2.v > delta * delta)
    sq = np.sqrt(np.where(beyond, chi2.v, 1))
    one = np.ones_like(sq)
    # beyond delta: rho = 2 sqrt(chi2) delta - delta^2, rho' = delta / sqrt(chi2); a relative error of chi2 is half that of its root
    rel = np.where(beyond, chi2.f / np.where(beyond, chi2.v, 1), 0) / 2 + 1
    rho = VM(*(np.where(beyond, a, b) for a, b in ((2 * sq * delta - delta * delta, chi2.v), (2 * np.sqrt(chi2.m) * delta + delta * delta, chi2.m),
                                                    (2 * sq * delta * (rel + 1) + np.abs(2 * sq * delta - delta * delta), chi2.f))))
    rho1 = VM(np.where(beyond, delta / sq, one), np.where(beyond, delta / sq, one), np.where(beyond, delta / sq * (rel + 1), 0 * one))
    W = rho1 * w
    Jl, Jp = jacobians(win, R, p, stereo, dt)
    act = active.astype(dt)
    free = active & (ph[ep] >= 0)
    fr = free.astype(dt)
    out = dict(hpose=hp, hpoint=hl, ph=ph[ep], lh=lh[el], active=active, free=free, beyond=beyond, depth=p[2].v, chi2_edge=chi2.v, dt=dt)

    def quad(J, n, mask):   # sum J^T W J -> [E, n, n] pairs
        return stack([[(J[0][r] * W * J[0][c] + J[1][r] * W * J[1][c] + J[2][r] * W * J[2][c]) * mask for c in range(n)] for r in range(n)])

    def grad(J, n, mask):   # -J^T rho' w e
        return tuple(a[:, 0] for a in stack([[-(J[0][r] * W * e[0] + J[1][r] * W * e[1] + J[2][r] * W * e[2]) * mask for r in range(n)]]))

    def scatter(pair, idx, n, sel):
        res = []
        for a in pair:
            t = np.zeros((n,) + a.shape[1:], dt)
            np.add.at(t, idx[sel], a[sel])   # (in index order: the edges' insertion order)
            res.append(t)
        return tuple(res)

    out["Hll"] = scatter(quad(Jl, 3, act), lh[el], n_l, active)
    out["b_l"] = scatter(grad(Jl, 3, act), lh[el], n_l, active)
    out["Hpp"] = scatter(quad(Jp, 6, fr), ph[ep], n_p, free)
    out["b_p"] = scatter(grad(Jp, 6, fr), ph[ep], n_p, free)
    out["B"] = stack([[(Jp[0][r] * W * Jl[0][c] + Jp[1][r] * W * Jl[1][c] + Jp[2][r] * W * Jl[2][c]) * fr for c in range(3)] for r in range(6)])
    out["chi2"] = tuple(dt((a * act).sum()) for a in (rho.v, rho.m, rho.f))
    diag = [np.concatenate([np.abs(out["Hpp"][k][:, range(6), range(6)]).ravel(), np.abs(out["Hll"][k][:, range(3), range(3)]).ravel()]) for k in range(3)]
    out["lambda"] = tuple(dt(1e-5) * d.max() for d in diag)
    return out


def reduce(lin, lam=None):
    """the Schur complement at lambda (None: lambda_init) -> dict quantity -> (value, scale M = m + f); Hs as [6 np, 6 np], bs [6 np]"""
    dt = lin["dt"]
    lam = lin["lambda"][0] if lam is None else dt(lam)
    n_p, n_l = len(lin["hpose"]), len(lin["hpoint"])
    I3 = np.eye(3, dtype=dt)
    Dinv = mat3_inverse(lin["Hll"][0] + lam * I3)
    aD = np.abs(Dinv)
    Dinv_m = aD + aD @ (lin["Hll"][1] + lin["Hll"][2] + lam * I3) @ aD   # (the conditioning of a nearly rank-2 landmark block)
    # value, m (absolute values, D^-1 replaced by Dinv_m), f (what the errors of B, b_l, Hpp, b_p become; D^-1's is in Dinv_m)
    Hs = [np.zeros((6 * n_p, 6 * n_p), dt) for _ in range(3)]
    bs = [lin["b_p"][k].reshape(-1).copy() for k in range(3)]
    for k in range(3):
        for i in range(n_p):
            Hs[k][6 * i:6 * i + 6, 6 * i:6 * i + 6] = lin["Hpp"][k][i] + (lam if k < 2 else 0) * np.eye(6, dtype=dt)
    order = np.argsort(lin["lh"], kind="stable")
    order = order[lin["free"][order]]
    cuts = np.nonzero(np.diff(lin["lh"][order]))[0] + 1
    for idx in np.split(order, cuts) if len(order) else []:
        l = lin["lh"][idx[0]]
        rows = (6 * lin["ph"][idx][:, None] + np.arange(6)).ravel()
        sq = lambda Y, Bm: np.einsum("aik,bjk->aibj", Y, Bm).reshape(len(rows), len(rows))
        Bv, Bm, Bf = (lin["B"][k][idx] for k in range(3))   # [m, 6, 3]
        aB = np.abs(Bv)
        blv, blm, blf = (lin["b_l"][k][l] for k in range(3))
        Hs[0][np.ix_(rows, rows)] -= sq(Bv @ Dinv[l], Bv)
        Hs[1][np.ix_(rows, rows)] += sq(Bm @ Dinv_m[l], Bm)
        Hs[2][np.ix_(rows, rows)] += sq(Bf @ aD[l], aB) + sq(aB @ aD[l], Bf)
        bs[0][rows] -= (Bv @ Dinv[l] @ blv).ravel()
        bs[1][rows] += (Bm @ Dinv_m[l] @ blm).ravel()
        bs[2][rows] += (Bf @ aD[l] @ np.abs(blv) + aB @ aD[l] @ blf).ravel()
    scaled = lambda t: (t[0], t[1] + t[2])
    return dict(Hll=scaled(lin["Hll"]), b_l=scaled(lin["b_l"]), Hpp=scaled(lin["Hpp"]), b_p=scaled(lin["b_p"]), Hs=scaled(Hs), bs=scaled(bs),
                lam=lam, **{"lambda": scaled(lin["lambda"]), "chi2": scaled(lin["chi2"])})


def reference(win, est, lam=None):
    return reduce(linearise(win, est, LD), lam)


def model_textbook(win, est, lam=None):
    """float64 model (a): the same explicit-block form, every operation in float64, edges in insertion order"""
    return reduce(linearise(win, est, np.float64), lam)


def model_records(win, est, lam=None):
    """float64 model (b), the factored form: one reciprocal per edge (a = x iz, b = y iz, iz = 1 / z), J_pose = Pt E, J_l = -iz Pt R with
    Pt = [fx 0 -a fx; 0 fy -b fy; (stereo) fx 0 bf iz - a fx], E = [[a b 1]x | -iz I], C = W iz Pt^T Pt, B = -E^T C R, and
    B_a D^-1 B_b^T = E_a^T Q E_b with Q = C_a (R_a D^-1 R_b^T) C_b; the own term of a diagonal item enters Q as -W Pt^T Pt."""
    f8 = np.float64
    lin = linearise(win, est, f8)   # (index structure, weights; the sums below are formed anew)
    fx, fy, cx, cy, bf = cam(win, f8)
    E_ = win["n_edges"]
    ep, el = np.asarray(win["edge_pose"]), np.asarray(win["edge_point"])
    pose, point = est["pose"].astype(f8), est["point"].astype(f8)
    R = rot_from_quat(pose[:, :4])[ep]
    p = np.einsum("eij,ej->ei", R, point[el]) + pose[ep, 4:7]
    st = np.asarray(win["edge_stereo"]).astype(bool)
    act, free = lin["active"], lin["free"]
    iz = 1.0 / p[:, 2]
    a, b = p[:, 0] * iz, p[:, 1] * iz
    z0 = np.zeros(E_)
    Pt = np.moveaxis(np.array([[fx + z0, z0, -a * fx], [z0, fy + z0, -b * fy], [np.where(st, fx, 0), z0, np.where(st, bf * iz - a * fx, 0)]]), -1, 0)
    Em = np.moveaxis(np.array([[z0, -1 + z0, b, -iz, z0, z0], [1 + z0, z0, -a, z0, -iz, z0], [-b, a, z0, z0, z0, -iz]]), -1, 0)
    # weights and residual as model (a) has them (the residual pass is not what differs between the forms)
    obs = np.asarray(win["edge_obs"], np.float32).astype(f8)
    pv = [VM(p[:, i]) for i in range(3)]
    e = np.stack([c.v for c in residual(win, pv, np.asarray(win["edge_obs"], np.float32), st.astype(np.uint8), f8)], 1)
    w = np.asarray(win["edge_inv_sigma2"], np.float32).astype(f8)
    chi2 = (e * e).sum(1) * w
    delta = np.where(st, DELTA[1], DELTA[0])
    beyond = np.asarray(est["e_robust"]).astype(bool) & (chi2 > delta * delta)
    sq = np.sqrt(np.where(beyond, chi2, 1.0))
    W = np.where(beyond, delta / sq, 1.0) * w * act
    rho = np.where(beyond, 2 * sq * delta - delta * delta, chi2)
    PtP = np.einsum("eki,ekj->eij", Pt, Pt)
    C = (W * iz)[:, None, None] * PtP
    Jl = -iz[:, None, None] * (Pt @ R)
    omr = -(W[:, None] * e)
    n_p, n_l = len(lin["hpose"]), len(lin["hpoint"])
    Hll, b_l = np.zeros((n_l, 3, 3)), np.zeros((n_l, 3))
    np.add.at(Hll, lin["lh"][act], np.einsum("eki,e,ekj->eij", Jl, W, Jl)[act])
    np.add.at(b_l, lin["lh"][act], np.einsum("eki,ek->ei", Jl, omr)[act])
    Wf = W * free
    Hpp, b_p = np.zeros((n_p, 6, 6)), np.zeros((n_p, 6))
    np.add.at(Hpp, lin["ph"][free], np.einsum("eki,ekl,elj->eij", Em, Wf[:, None, None] * PtP, Em)[free])
    np.add.at(b_p, lin["ph"][free], np.einsum("eki,elk,el->ei", Em, Pt, omr * free[:, None])[free])
    diag = np.concatenate([np.abs(Hpp[:, range(6), range(6)]).ravel(), np.abs(Hll[:, range(3), range(3)]).ravel()])
    lam_init = 1e-5 * diag.max()
    lam = lam_init if lam is None else f8(lam)
    Dinv = mat3_inverse(Hll + lam * np.eye(3))
    # items: (landmark, free edges ea <= eb by keyframe hidx)
    fe = np.nonzero(free)[0]
    fe = fe[np.lexsort((lin["ph"][fe], lin["lh"][fe]))]
    lhs = lin["lh"][fe]
    ia, ib = [], []
    for idx in np.split(fe, np.nonzero(np.diff(lhs))[0] + 1) if len(fe) else []:
        u, v = np.triu_indices(len(idx))
        ia.append(idx[u]); ib.append(idx[v])
    ia, ib = (np.concatenate(x) if x else np.zeros(0, int) for x in (ia, ib))
    Cf = C * free[:, None, None]
    G = np.einsum("nij,njk,nlk->nil", R[ia], Dinv[lin["lh"][ia]], R[ib])
    Q = Cf[ia] @ G @ Cf[ib]
    same = ia == ib
    Q = Q - np.where(same, Wf[ia], 0.0)[:, None, None] * PtP[ia]
    blk = np.einsum("nki,nkl,nlj->nij", Em[ia], Q, Em[ib])
    Hs = np.zeros((n_p, n_p, 6, 6))
    np.add.at(Hs, (lin["ph"][ia], lin["ph"][ib]), -blk)
    off = ~same
    np.add.at(Hs, (lin["ph"][ib][off], lin["ph"][ia][off]), -np.swapaxes(blk[off], 1, 2))
    Hs = Hs.transpose(0, 2, 1, 3).reshape(6 * n_p, 6 * n_p) + lam * np.eye(6 * n_p)
    t = np.einsum("eij,ej->ei", R @ Dinv[lin["lh"]], b_l[lin["lh"]])       # R_a D^-1 b_l
    coef = -np.einsum("eki,ekl,el->ei", Em, Cf, t)                         # B_a D^-1 b_l
    sb = np.zeros((n_p, 6))
    np.add.at(sb, lin["ph"][free], coef[free])
    bs = (b_p - sb).ravel()
    pair = lambda x: (x, None)
    return dict(Hll=pair(Hll), b_l=pair(b_l), Hpp=pair(Hpp), b_p=pair(b_p), Hs=pair(Hs), bs=pair(bs), lam=lam,
                **{"lambda": pair(lam_init), "chi2": pair((rho * act).sum())})


# ------------------------------------------------------------------------------------------ the measure
def split_hs(Hs, n_p):
    """[6 np, 6 np] -> blocks [np, np, 6, 6]"""
    return np.asarray(Hs).reshape(n_p, 6, n_p, 6).transpose(0, 2, 1, 3)


def omegas(ref, got):
    """got: dict quantity -> array (Hll, b_l, Hpp, b_p, Hs [6 np, 6 np], bs, lambda, chi2; a missing one is skipped) ->
    dict quantity -> (worst omega, index of the worst entry); Hs is reported as Hs_diag / Hs_off with block indices (i1, i2, r, c)"""
    n_p = len(ref["Hpp"][0])
    out = {}

    def put(name, g, v, m):
        g, v, m = np.asarray(g, LD), np.asarray(v, LD), np.asarray(m, LD)
        if g.size == 0:
            return
        d = np.abs(g - v)
        om = np.where(d == 0, LD(0), d / (U53 * np.where(m > 0, m, LD("1e-4000"))))
        k = np.unravel_index(int(np.argmax(om)), om.shape) if om.ndim else ()
        out[name] = (float(om[k]), tuple(int(x) for x in k))

    for name in ("Hll", "b_l", "Hpp", "b_p", "bs", "lambda", "chi2"):
        if name in got:
            put(name, got[name], *ref[name])
    if "Hs" in got:
        g, v, m = (split_hs(x, n_p) for x in (got["Hs"], ref["Hs"][0], ref["Hs"][1]))
        dg = np.eye(n_p, dtype=bool)
        put("Hs_diag", g[dg], v[dg], m[dg])
        if n_p > 1:
            i1, i2 = np.nonzero(~dg)
            put("Hs_off", g[i1, i2], v[i1, i2], m[i1, i2])
            if "Hs_off" in out:
                om, k = out["Hs_off"]
                out["Hs_off"] = (om, (int(i1[k[0]]), int(i2[k[0]])) + k[1:])
    return out


def model_omegas(win, est, lam=None, ref=None):
    """worst omega of the two float64 models per quantity -> (dict quantity -> max over the models, dict model -> its omegas)"""
    ref = reference(win, est, lam) if ref is None else ref
    per = {}
    for name, f in (("textbook", model_textbook), ("records", model_records)):
        mdl = f(win, est, lam)
        per[name] = omegas(ref, {q: mdl[q][0] for q in ("Hll", "b_l", "Hpp", "b_p", "Hs", "bs", "lambda", "chi2")})
    worst = {q: max(per[n][q][0] for n in per if q in per[n]) for q in QUANTITIES if any(q in per[n] for n in per)}
    return worst, per


# ------------------------------------------------------------------------------------------ hand-built windows
CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448)


def rotvec_to_R(r):
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def qt_from_Tcw(T):
    """Converter::toSE3Quat: float32 4 x 4 -> qx qy qz qw tx ty tz (Eigen's matrix -> quaternion)"""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    m = T[:3, :3]
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        q = [(m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s, w]
    else:
        i = int(np.argmax(np.diag(m)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q = [0.0] * 4
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    q = np.array(q)
    q /= np.linalg.norm(q)
    return np.concatenate([q, T[:3, 3]])


def host_estimates(win, masked=None, robust=True):
    """the estimates a first linearisation starts from, as the CPU tests form them (the GPU tests take the tap's)"""
    E = win["n_edges"]
    lv = np.zeros(E, np.uint8)
    if masked is not None:
        lv[np.asarray(masked)] = 1
    return dict(pose=np.stack([qt_from_Tcw(T) for T in win["pose_Tcw"]]), point=np.asarray(win["point_xyz"], np.float32).astype(np.float64),
                e_level1=lv, e_robust=np.full(E, 1 if robust else 0, np.uint8))


def make_window(seed, n_free, n_fixed, sees, kinds="mixed", huber_split=True, noise=None, perturb=0.0, outliers=(), mono_only=(), depths=(0.6, 40.0)):
    """A window whose structure is given: sees[l] = the keyframes (0 .. n_free - 1 free, then fixed) that observe landmark l.
    Keyframes at |t| up to 10 with small rotations, depths 0.5 .. 50, observations = the projection at the float32 estimates plus a
    residual of chosen size: huber_split draws w |e|^2 on both sides of the Huber delta (half the edges at 0.2-2, half at 3-8
    standard deviations), else `noise` standard deviations.  perturb: the estimates then move away from where the observations were
    made (a window for an optimisation).  outliers: edge indices that get +-60 .. 200 px.  kinds: mono / stereo / mixed."""
    rng = np.random.default_rng(seed)
    n_poses, n_points = n_free + n_fixed, len(sees)
    Tcw = np.zeros((n_poses, 4, 4), np.float32)
    for i in range(n_poses):
        Rm = rotvec_to_R(rng.uniform(-0.03, 0.03, 3))
        c = np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), -rng.uniform(0, 8)])
        Tcw[i, :3, :3] = Rm
        Tcw[i, :3, 3] = -Rm @ c
        Tcw[i, 3, 3] = 1
    Td = Tcw.astype(np.float64)
    pts = np.zeros((n_points, 3))
    for l, ks in enumerate(sees):
        ks = list(ks)
        depth = 10 ** rng.uniform(np.log10(depths[0]), np.log10(depths[1]))
        cen = np.mean([-Td[k, :3, :3].T @ Td[k, :3, 3] for k in ks], 0)
        X = cen + np.array([rng.uniform(-0.3, 0.3) * depth, rng.uniform(-0.3, 0.3) * depth, 0])
        zc = max(-(Td[k, :3, :3].T @ Td[k, :3, 3])[2] for k in ks)
        X[2] = zc + depth
        for _ in range(4):   # every depth within 0.5 .. 50
            d = np.array([(Td[k, :3, :3] @ X + Td[k, :3, 3])[2] for k in ks])
            if d.min() < 0.55:
                X[2] += 0.6 - d.min()
        pts[l] = X
    pts32 = pts.astype(np.float32)
    ep, el = [], []
    for l, ks in enumerate(sees):
        for k in ks:
            ep.append(k); el.append(l)
    ep, el = np.array(ep, np.int32), np.array(el, np.int32)
    E = len(ep)
    if kinds == "mono":
        stereo = np.zeros(E, np.uint8)
    elif kinds == "stereo":
        stereo = np.ones(E, np.uint8)
    else:
        stereo = (rng.uniform(size=E) < 0.5).astype(np.uint8)
    for l in mono_only:
        stereo[el == l] = 0
    w = (1.2 ** (-2.0 * rng.integers(0, 8, E))).astype(np.float32)
    P = pts32.astype(np.float64)
    pc = np.einsum("eij,ej->ei", Td[ep, :3, :3], P[el]) + Td[ep, :3, 3]
    fx, fy, cx, cy, bf = (float(np.float32(CAM[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
    u, v = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
    proj = np.stack([u, v, u - bf / pc[:, 2]], 1)
    if huber_split:
        size = np.where(rng.uniform(size=E) < 0.5, rng.uniform(0.2, 2.0, E), rng.uniform(3.0, 8.0, E))
    else:
        size = np.abs(rng.normal(0, noise if noise is not None else 0.7, E))
    dirn = rng.normal(size=(E, 3))
    dirn[stereo == 0, 2] = 0
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    obs = proj + dirn * (size / np.sqrt(w.astype(np.float64)))[:, None]
    for e_ in outliers:
        obs[e_, :2] += rng.choice([-1.0, 1.0], 2) * rng.uniform(60, 200, 2)
        obs[e_, 2] = obs[e_, 0] - (proj[e_, 0] - proj[e_, 2])
    obs[stereo == 0, 2] = -1.0
    if perturb:
        for i in range(n_free):
            dR = rotvec_to_R(rng.normal(0, perturb * 0.01, 3))
            Td[i, :3, :3] = dR @ Td[i, :3, :3]
            Td[i, :3, 3] = dR @ Td[i, :3, 3] + rng.normal(0, perturb * 0.02, 3)
        P = P + rng.normal(0, perturb * 0.02, P.shape) * (1 + 0.02 * np.abs(P[:, 2:3]))
    fixed = np.zeros(n_poses, np.uint8)
    fixed[n_free:] = 1
    win = dict(n_poses=n_poses, n_points=n_points, n_edges=E, pose_Tcw=Td.astype(np.float32).reshape(n_poses, 16), pose_fixed=fixed,
               pose_id=np.arange(n_poses, dtype=np.int64) + 1, point_xyz=P.astype(np.float32), point_id=np.arange(n_points, dtype=np.int64) + 100,
               edge_pose=ep, edge_point=el, edge_obs=obs.astype(np.float32), edge_stereo=stereo, edge_inv_sigma2=w, **CAM)
    return win


# ---- which landmark is seen by which keyframe: the structures of the test cases
COUNTS = (0, 1, 15, 16, 17, 32, 33, 255, 256, 257, 600)


def sees_counts(n_co):
    """np = 2 plus two fixed keyframes: n_co landmarks seen by both free keyframes (and fixed ones), some seen by one only"""
    s = [[0, 1, 2 + l % 2] for l in range(n_co)]
    s += [[0, 2, 3] for _ in range(5)] + [[1, 2] for _ in range(4)] + [[1, 3] for _ in range(3)]
    return s


PACK_NP = 7
# item counts of the 21 off-diagonal blocks of np = 7 in rank order: empty blocks first, in the middle and last; 5 + 5 + 5 rows and
# then a 3-row block that would straddle the unit (padded); 16-row blocks arriving at in_unit = 0 and at in_unit > 0; a partial last unit
PACK_COUNTS = (0, 70, 80, 75, 40, 0, 250, 256, 3, 241, 16, 17, 0, 0, 1, 100, 31, 33, 200, 9, 0)


def pairs_upper(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def sees_pack():
    s = []
    for (i, j), n in zip(pairs_upper(PACK_NP), PACK_COUNTS):
        s += [[i, j, PACK_NP + l % 2] for l in range(n)]
    return s


DIAG_OBS = (1, 255, 256, 257, 1025)


def sees_diag():
    """five free keyframes with 1, 255, 256, 257, 1025 observations, each landmark also seen by a fixed keyframe"""
    s = []
    for i, n in enumerate(DIAG_OBS):
        s += [[i, 5 + l % 2] for l in range(n)]
    return s


SIZES = (1, 3, 8, 40, 41, 43)


def sees_size(n_free, rng):
    """every free keyframe linked to its neighbours (and a few far ones), two fixed keyframes; ~12 landmarks per keyframe"""
    s = []
    for i in range(n_free):
        for r in range(6):
            ks = {i, n_free + r % 2}
            if n_free > 1:
                ks.add((i + 1 + r % 3) % n_free)
            if r == 5 and n_free > 8:
                ks.add(int(rng.integers(0, n_free)))
            s.append(sorted(ks))
    return s


DEGREES = (1, 2, 4, 5, 6, 7, 8, 9, 17, 40)


def sees_degree(rng):
    """40 free + 5 fixed keyframes; landmarks of every degree in DEGREES on free keyframes, plus a landmark seen only by fixed
    keyframes and one seen by one free and several fixed.  -> (sees, indices of the degree-1 landmarks: mono only)"""
    s, mono = [], []
    for d in DEGREES:
        for r in range(6 if d < 17 else 3):
            ks = sorted(int(k) for k in rng.choice(40, d, replace=False))
            if d == 1:
                mono.append(len(s))
            elif r % 2:
                ks.append(40 + r % 5)
            s.append(ks)
    s.append([40, 41, 42])
    s.append([41, 43])
    s.append([7, 40, 41, 42, 44])
    s.append([39, 40, 43, 44])
    for i in range(40):   # every keyframe keeps enough observations for a well-posed block
        s.append([i, (i + 1) % 40, 40 + i % 5])
        s.append([i, (i + 3) % 40])
        s.append([i, (i + 1) % 40, (i + 2) % 40])
    return s, mono


def unit_kinds(blk_off, n_p):
    """build_schur_units restated: -> (kind of every block {(i1, i2): 'DIAG' | 'BIG' | 'PACK'}, item counts, number of PACK units,
    per PACK block (i1, i2, rows, in_unit on arrival, the unit was padded for it))"""
    kinds, counts, trace = {}, {}, []
    in_unit, n_pack, blk = 0, 0, 0
    for i1 in range(n_p):
        for i2 in range(i1, n_p):
            n = int(blk_off[blk + 1] - blk_off[blk])
            blk += 1
            counts[(i1, i2)] = n
            if i1 == i2:
                kinds[(i1, i2)] = "DIAG"
                continue
            if n > 256:
                kinds[(i1, i2)] = "BIG"
                continue
            kinds[(i1, i2)] = "PACK"
            rows = max(1, (n + 15) // 16)
            trace.append((i1, i2, rows, in_unit, in_unit + rows > 16))
            if in_unit + rows > 16:
                in_unit = 0
            if in_unit == 0:
                n_pack += 1
            in_unit = (in_unit + rows) % 16
    return kinds, counts, n_pack, trace


# ---- the inputs of the GPU tests, by family (tests/test_lba_system_cpu.py runs the float64 models on every one of them)
LAMBDA_FACTORS = (1e-8, 1.0, 1e4)
_cache = {}


def stage1_window(seed):
    """a window for the second optimisation's system: observations within a fraction of a pixel, estimates moved away from them, and
    gross outliers planted: every observation of landmark 0, every observation of the lightly observed free keyframe 5, 3 % of the
    observations of landmarks seen five times or more.  -> (window, planted edges)"""
    rng = np.random.default_rng(seed)
    n_free, n_fixed = 6, 3
    sees = []
    for l in range(150):
        ks = sorted(int(k) for k in rng.choice(5, int(rng.integers(3, 6)), replace=False))
        if l % 2 == 0:
            ks.append(n_free + l % n_fixed)
        sees.append(ks)
    sees[0] = [0, 2, 3, n_free]
    for l in (7, 31, 64, 90):   # keyframe 5: four observations
        sees[l] = sorted(set(sees[l]) | {5})
    ep = np.array([k for ks in sees for k in ks])
    el = np.array([l for l, ks in enumerate(sees) for _ in ks])
    deg = np.array([len(ks) for ks in sees])
    planted = (el == 0) | (ep == 5) | ((rng.uniform(size=len(ep)) < 0.03) & (deg[el] >= 5))
    out = np.nonzero(planted)[0]
    return make_window(seed, n_free, n_fixed, sees, huber_split=False, noise=0.5, perturb=0.03, outliers=out, depths=(3.0, 40.0)), out


def cases(family):
    """-> list of dicts: name, win, stage, lam_factor (None: lambda_init), planted (stage 1)"""
    if family in _cache:
        return _cache[family]
    c = lambda name, win, **kw: dict(dict(name=name, win=win, stage=0, lam_factor=None, planted=None, family=family), **kw)
    if family == "counts":
        out = [c("co%d" % n, make_window(100 + n, 2, 2, sees_counts(n))) for n in COUNTS]
    elif family == "pack":
        out = [c("pack", make_window(201, PACK_NP, 2, sees_pack()))]
    elif family == "diag":
        out = [c("diag", make_window(301, len(DIAG_OBS), 2, sees_diag()))]
    elif family == "sizes":
        out = [c("np%d" % q, make_window(400 + q, q, 2, sees_size(q, np.random.default_rng(q)))) for q in SIZES]
    elif family == "degree":
        s, mono = sees_degree(np.random.default_rng(5))
        out = [c("degree", make_window(501, 40, 5, s, mono_only=mono))]
    elif family == "kinds":
        out = [c(k, make_window(600 + i, 8, 2, sees_size(8, np.random.default_rng(8)), kinds=k)) for i, k in enumerate(("mono", "stereo", "mixed"))]
    elif family == "lambda":
        out = [dict(b, name="%s x%g" % (b["name"], f), lam_factor=f, family=family) for b in cases("counts") + cases("degree") for f in LAMBDA_FACTORS]
    elif family == "stage1":
        out = []
        for seed in (704, 708, 709):   # (seeds at which the oracle masks exactly the planted edges and accepts every step: test_lba_system_cpu)
            win, planted = stage1_window(seed)
            out.append(c("s1_%d" % seed, win, stage=1, planted=planted))
    else:
        raise KeyError(family)
    _cache[family] = out
    return out


FAMILIES = ("counts", "pack", "diag", "sizes", "degree", "kinds", "lambda", "stage1")


def evaluate(case, est, lam=None):
    """reference and the worst omegas of the float64 models of a case at the estimates `est` (the linearisations are kept: the lambda family
    revisits the windows of two others) -> (ref, worst per quantity, per model)"""
    key = (id(case["win"]), est["pose"].tobytes(), est["e_level1"].tobytes(), est["e_robust"].tobytes())
    if key not in _cache:
        _cache[key] = linearise(case["win"], est, LD)
    lin = _cache[key]
    if case["lam_factor"] is not None and lam is None:
        lam = float(lin["lambda"][0]) * case["lam_factor"]
    ref = reduce(lin, lam)
    worst, per = model_omegas(case["win"], est, lam, ref=ref)
    return ref, worst, per
