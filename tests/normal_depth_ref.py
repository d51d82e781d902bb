"""MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:363-413) with compute_std_pts (:27-37) and the planner's map rows
(src/Planning.cc:86-96, src/Tracking.cc:1088-1112) restated with numpy scalars, one operation at a time with the type each operand
has in the reference under the conventions of DESIGN.md section 2 item 21: np.float32 where the reference computes in float,
np.float64 where it computes in double, every association written out.  Independent of csrc/normal_depth.h: it shares no code with
the library and is what the host tap and the device are compared with, bit for bit."""
import numpy as np

F, D = np.float32, np.float64
UPDATED, BAD, NO_OBS, UNKNOWN, REF_UNUSABLE = range(5)
ROWS_PLANNING, ROWS_TRACKING = 0, 1
OUTPUTS = (("status", np.uint8, 1), ("normal", np.float32, 3), ("min_dist", np.float32, 1), ("max_dist", np.float32, 1),
           ("theta_mean", np.float32, 1), ("theta_std", np.float32, 1), ("n_terms", np.int32, 1), ("upper", np.float32, 1),
           ("lower", np.float32, 1), ("max_range", np.float32, 1), ("min_range", np.float32, 1))


def norm(d):
    """cv::norm of a 3x1 float matrix: the squares summed in double in index order, the root in double"""
    s = (D(d[0]) * D(d[0]) + D(d[1]) * D(d[1])) + D(d[2]) * D(d[2])
    return np.sqrt(s)


def term(P, O):
    """:388-394 for one observer -> (normali / cv::norm(normali) as three floats, theta)"""
    d = [F(P[c]) - F(O[c]) for c in range(3)]
    inv = F(D(1.0) / norm(d))
    u = [d[c] * inv for c in range(3)]
    theta = F(np.arctan2(D(d[0]), D(d[2])))
    return u, theta


def compute_std_pts(v):
    """:27-37: accumulate and inner_product start from the double 0.0, so they add in double; the results land in floats"""
    acc = D(0.0)
    for t in v:
        acc = acc + D(t)
    total = F(acc)
    mean = total / F(len(v))
    acc = D(0.0)
    for t in v:
        diff = F(t) - mean
        acc = acc + D(diff * diff)   # a float product, added in double
    sq_sum = F(acc)
    return mean, np.sqrt(sq_sum / F(len(v)))


def rows(form, mean, std, min_dist, max_dist):
    """-> upper, lower, max_range, min_range"""
    wide = D(std) * D(2.5)
    if form == ROWS_PLANNING:   # theta_interval is a float member
        iv = F(30.0 / 57.3) if wide < D(30.0 / 57.3) else F(wide)
        upper, lower = mean + iv, mean - iv
    else:                       # a double local
        iv = D(10.0 / 57.3) if wide < D(10.0 / 57.3) else wide
        upper, lower = F(D(mean) + iv), F(D(mean) - iv)
    return upper, lower, F(1.2) * max_dist, F(0.8) * min_dist


def one_point(g, v, row, P, ref_kf, kf_center, scale):
    """-> (status, None) or (UPDATED, dict(normal, min_dist, max_dist, theta_mean, theta_std, units, thetas))"""
    if row >= g["n_points"]:
        return UNKNOWN, None
    if g["point_bad"][row]:
        return BAD, None
    e0, e1 = int(g["obs_off"][row]), int(g["obs_off"][row + 1])
    if e1 == e0:
        return NO_OBS, None
    normal = [F(0.0)] * 3
    units, thetas, observations = [], [], {}
    for e in range(e0, e1):   # the stored order of the row
        kf = int(g["obs_kf"][e])
        observations[kf] = int(v["obs_idx"][e])
        u, theta = term(P, kf_center[kf])
        normal = [normal[c] + u[c] for c in range(3)]
        units.append(u)
        thetas.append(theta)
    n = e1 - e0
    idx = observations.get(ref_kf, 0)   # map::operator[] of a key that is not there
    f0, f1 = int(g["kf_mp_off"][ref_kf]), int(g["kf_mp_off"][ref_kf + 1])
    if idx >= f1 - f0:
        return REF_UNUSABLE, None
    level = int(v["kf_octave"][f0 + idx])
    if level < 0 or level >= len(scale):
        return REF_UNUSABLE, None
    dist = F(norm([F(P[c]) - F(kf_center[ref_kf][c]) for c in range(3)]))
    max_dist = dist * F(scale[level])
    min_dist = max_dist / F(scale[len(scale) - 1])
    k = F(D(1.0) / D(n))
    mean, std = compute_std_pts(thetas)
    return UPDATED, dict(normal=[normal[c] * k for c in range(3)], min_dist=min_dist, max_dist=max_dist, theta_mean=mean, theta_std=std,
                         n_terms=n, units=units, thetas=thetas)


def update_normal_depth(g, v, point, xyz, ref_kf, kf_center, scale, rows_form=ROWS_PLANNING, term_off=None):
    """the batch -> the outputs of aos2_local_map_update_normal_depth as arrays PRESET to the sentinel the binding uses (status 255,
    n_terms -7, floats -7.0): what a point that is not updated leaves behind; term_unit / term_theta only with term_off"""
    n = len(point)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    kf_center = np.asarray(kf_center, np.float32).reshape(-1, 3)
    scale = np.asarray(scale, np.float32)
    out = {k: np.full((n, per) if per == 3 else n, 255 if dt == np.uint8 else -7, dt) for k, dt, per in OUTPUTS}
    if term_off is not None:
        out["term_unit"] = np.full((int(term_off[-1]), 3), -7, np.float32)
        out["term_theta"] = np.full(int(term_off[-1]), -7, np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            st, r = one_point(g, v, int(point[i]), xyz[i], int(ref_kf[i]), kf_center, scale)
            out["status"][i] = st
            if st != UPDATED:
                continue
            for k in ("normal", "min_dist", "max_dist", "theta_mean", "theta_std", "n_terms"):
                out[k][i] = r[k]
            out["upper"][i], out["lower"][i], out["max_range"][i], out["min_range"][i] = rows(
                rows_form, r["theta_mean"], r["theta_std"], r["min_dist"], r["max_dist"])
            if term_off is not None and term_off[i + 1] - term_off[i] == r["n_terms"]:
                a = int(term_off[i])
                out["term_unit"][a:a + r["n_terms"]] = r["units"]
                out["term_theta"][a:a + r["n_terms"]] = r["thetas"]
    return out
