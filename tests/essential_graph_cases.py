"""What the essential-graph tests share beside the restatement (tests/essential_graph_ref.py): the closed-form Jacobian of the edge's
residual, the inputs the generator never produces (`turned`: edges in both orientations between free vertices, a free pair named
twice, the fixed vertex anywhere) and a plain replay of constructQuadraticForm over the edges (`replay`) that uses nothing of the
library's lists."""
import os

import numpy as np

import essential_graph_ref as R

DBL_EPSILON = 2.0 ** -52


# ---------------------------------------------------------------------------------------------- the closed-form Jacobian
def adjoint(S):
    """S exp(u) S^-1 = exp(Ad u) for u = (omega, upsilon, sigma): omega' = R omega, upsilon' = s R upsilon + t x R omega - sigma t"""
    Rm = R.rot_of((S[:4] / np.linalg.norm(S[:4]))[None])[0]
    t, s = S[4:7], S[7]
    Ad = np.zeros((7, 7))
    Ad[:3, :3] = Rm
    Ad[3:6, :3] = R.S3.skew(t) @ Rm
    Ad[3:6, 3:6] = s * Rm
    Ad[3:6, 6] = -t
    Ad[6, 6] = 1
    return Ad


def small_adjoint(xi):
    """ad_xi: the derivative of Ad(exp(h xi)) at h = 0"""
    w, v, sg = xi[:3], xi[3:6], xi[6]
    ad = np.zeros((7, 7))
    ad[:3, :3] = R.S3.skew(w)
    ad[3:6, :3] = R.S3.skew(v)
    ad[3:6, 3:6] = R.S3.skew(w) + sg * np.eye(3)
    ad[3:6, 6] = -v
    return ad


def inverse_left_jacobian(xi):
    """log(exp(v) exp(xi)) = xi + Jl^-1(xi) v + O(v^2), Jl^-1 = sum B_n / n! ad^n (Bernoulli numbers, B_1 = -1/2)"""
    bern = [1.0, -0.5, 1 / 6, 0, -1 / 30, 0, 1 / 42, 0, -1 / 30, 0, 5 / 66, 0, -691 / 2730, 0, 7 / 6]
    ad, term, out, fact = small_adjoint(xi), np.eye(7), np.zeros((7, 7)), 1.0
    for n, Bn in enumerate(bern):
        if n:
            term, fact = term @ ad, fact * n
        out += Bn / fact * term
    return out


def closed_form(P, est):
    """the Jacobians of every edge in closed form (test_central_difference_jacobian_agrees_with_the_closed_form: d e / d u_i =
    Jl^-1(e) Ad_C, d e / d u_j = -Jl^-1(e) Ad_T with T = C S_i S_j^-1) -> J [ne][2][7][7], the bound of that test per edge
    100 M DBL_EPSILON / delta [ne] (M = max(1, the largest |t| among C, S_i, S_j^-1, T)), the largest |e|"""
    v0, v1, C = P["v0"], P["v1"], P["Sji"]
    inv = R.inverse(est)
    T = R.mul(R.mul(C, est[v0]), inv[v1])
    e = R.log(T)
    J = np.zeros((len(v0), 2, 7, 7))
    for k in range(len(v0)):
        Jl = inverse_left_jacobian(e[k])
        J[k, 0], J[k, 1] = Jl @ adjoint(C[k]), -Jl @ adjoint(T[k])
    M = np.maximum(1.0, np.max(np.abs(np.stack([C[:, 4:7], est[v0][:, 4:7], inv[v1][:, 4:7], T[:, 4:7]])), axis=(0, 2)))
    return J, 100 * M * DBL_EPSILON / R.DELTA, float(np.abs(e).max()) if len(e) else 0.0


def residual_bound(P, est):
    """test_header_residual_agrees_with_the_restatement's bound on a residual: 128 DBL_EPSILON M, M = max(1, the largest |t| among
    the measurements, the estimates and their inverses)"""
    M = max(1.0, np.abs(P["Sji"][:, 4:7]).max(), np.abs(est[:, 4:7]).max(), np.abs(R.inverse(est)[:, 4:7]).max())
    return 128 * DBL_EPSILON * M


# ---------------------------------------------------------------------------------------------- inputs the generator does not produce
def with_edges(P, ne):
    """P with `ne` edges: covisibility edges (kind 3) are dropped from the end; the spanning tree keeps the graph connected"""
    keep = np.ones(len(P["v0"]), bool)
    for e in range(len(keep) - 1, -1, -1):
        if keep.sum() == ne:
            break
        if P["kind"][e] == 3:
            keep[e] = False
    if keep.sum() != ne:
        raise ValueError("not enough covisibility edges to drop")
    return dict(P, v0=P["v0"][keep], v1=P["v1"][keep], Sji=P["Sji"][keep], kind=P["kind"][keep])


def with_residuals(P, seed):
    """P with measurements that leave a chosen residual on every edge, Sji = exp(xi) S_v1 S_v0^-1 with |xi| of 0.05 rad, 0.1 m and
    0.02 per component.  The generator's own measurements at 300 keyframes leave residuals of a metre where the loop correction (4 %
    of scale on a circle of 24 m) meets the uncorrected chain; the bounds used on the Jacobians are derived for |e| < 0.5."""
    rng = np.random.default_rng([seed, len(P["v0"])])
    S = np.asarray(P["Scw"], np.float64)
    xi = np.clip(rng.normal(size=(len(P["v0"]), 7)), -3, 3) * np.array([0.05, 0.05, 0.05, 0.1, 0.1, 0.1, 0.02])
    E = np.stack([R.exp1(u) for u in xi])
    return dict(P, Sji=R.mul(E, R.mul(S[P["v1"]], R.inverse(S)[P["v0"]])))


def turned(P, seed, fixed, residuals=False):
    """P as a caller may gather it as well: about half of the edges name their vertices the other way round (v0 and v1 swapped, the
    measurement inverted -- LoopConnections is a map of sets of pointers, and spanning-tree parents change after culling), the fixed
    vertex is `fixed`, and one free pair (a, b), a < b, is appended twice, as (b, a) and as (a, b), each measurement formed from the
    estimates (Sji = S_v1 S_v0^-1): one slot of H that receives J0^T J1 and J1^T J0 terms together.  residuals: the turned edges get
    the measurements of with_residuals."""
    n, ne = len(P["Scw"]), len(P["v0"])
    rng = np.random.default_rng([seed, n, ne, fixed])
    swap = rng.random(ne) < 0.5
    if ne >= 2:
        swap[rng.integers(ne)] = True      # at least one of each, whatever the draw
        swap[(np.flatnonzero(swap)[0] + 1) % ne] = False
    v0, v1 = np.where(swap, P["v1"], P["v0"]).astype(np.int32), np.where(swap, P["v0"], P["v1"]).astype(np.int32)
    Sji = np.where(swap[:, None], R.inverse(P["Sji"]), P["Sji"]) if ne else P["Sji"]
    kind = np.array(P["kind"])
    if residuals:
        Sji = with_residuals(dict(P, v0=v0, v1=v1), seed)["Sji"]
    free = [v for v in range(n) if v != fixed]
    if len(free) >= 2:
        a, b = sorted(rng.choice(free, 2, replace=False).tolist())
        S = np.asarray(P["Scw"], np.float64)
        m_ba, m_ab = R.mul(S[a:a + 1], R.inverse(S[b:b + 1])), R.mul(S[b:b + 1], R.inverse(S[a:a + 1]))
        v0, v1 = np.concatenate([v0, [b, a]]).astype(np.int32), np.concatenate([v1, [a, b]]).astype(np.int32)
        Sji, kind = np.concatenate([Sji, m_ba, m_ab]), np.concatenate([kind, [3, 3]])
    return dict(P, v0=v0, v1=v1, Sji=Sji, kind=kind, fixed=int(fixed))


SEED = 3
# n, fix_scale, fixed: the cases that are optimised; at 300 ne = 1496 and nf = 299 pass 256, so every strided loop wraps
OPTIMISED = ((9, False, 0), (9, True, 8), (17, False, 16), (65, True, 30), (65, False, 0))
_CASES = {}


def cases():
    """name -> problem, in a fixed order.  The first five are OPTIMISED; the rest is for the linearisation and the trial alone."""
    if not _CASES:
        for n, fix, fixed in OPTIMISED:
            _CASES["n%d_fix%d_fixed%d" % (n, fix, fixed)] = turned(R.problem(SEED, n, fix), SEED, fixed)
        _CASES["n300_fix0_fixed1"] = turned(R.problem(SEED, 300, False), SEED, 1, residuals=True)
        _CASES["n2_single_edge"] = turned(R.problem(SEED, 2, True), SEED, 0)
        _CASES["n3_free_pair"] = turned(R.problem(SEED, 3, False), SEED, 1)
        big = R.problem(SEED, 64, False)
        _CASES["ne256"] = turned(with_edges(big, 254), SEED, 63)
        _CASES["ne257"] = turned(with_edges(big, 255), SEED, 20)
    return _CASES


_OPTIMISED = {}


def optimised():
    """the OPTIMISED cases with the restatement's results and the measured resolution of each, as R.generator_case.  Once per process."""
    if not _OPTIMISED:
        names = list(cases())[:len(OPTIMISED)]
        problems = [cases()[k] for k in names]
        want = [R.optimize(P) for P in problems]
        res = []
        for P, w in zip(problems, want):
            r, same_status = R.resolution(P, w)
            if not same_status:
                raise RuntimeError("the re-associations disagree on the status")
            res.append(r)
        _OPTIMISED.update(names=names, problems=problems, want=want, resolution=res)
    return _OPTIMISED


TAPS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "essential_graph_taps.txt")
TAPS_HEAD = ["# OptimizeEssentialGraph: the device taps against their references (tests/test_essential_graph_linearised_gpu.py,",
             "# tests/test_essential_graph_trial_gpu.py), one line per case: the worst difference / bound of every comparison (<= 1 passes);",
             "# comparisons that are bit for bit are named as such"]


def record(key, text):
    """keep `key: text` in profiles/essential_graph_taps.txt (the other lines stay)"""
    lines = {}
    if os.path.exists(TAPS_FILE):
        with open(TAPS_FILE) as f:
            for ln in f.read().splitlines():
                if ln and not ln.startswith("#") and ": " in ln:
                    lines[ln.split(": ", 1)[0]] = ln.split(": ", 1)[1]
    lines[key] = text
    with open(TAPS_FILE, "w") as f:
        f.write("\n".join(TAPS_HEAD + ["%s: %s" % kv for kv in sorted(lines.items())]) + "\n")


def worst(diff, bound):
    """the largest diff / bound over the entries with a bound > 0 (0.0 when there is none)"""
    diff, bound = np.broadcast_arrays(np.asarray(diff, np.float64), np.asarray(bound, np.float64))
    m = bound > 0
    return float((diff[m] / bound[m]).max()) if m.any() else 0.0


def hessian_index(P):
    """vertex -> index among the free vertices in ascending order, -1 for the fixed one"""
    n = len(P["Scw"])
    h = np.cumsum(np.arange(n) != P["fixed"]) - 1
    h[P["fixed"]] = -1
    return h


def free_pairs(P):
    """edges with both ends free: how many have vertex 0 at the higher hessian index (J0^T J1 terms) and how many at the lower"""
    h = hessian_index(P)
    a, b = h[P["v0"]], h[P["v1"]]
    both = (a >= 0) & (b >= 0)
    return int((both & (a > b)).sum()), int((both & (a < b)).sum())


# ---------------------------------------------------------------------------------------------- constructQuadraticForm, replayed
def _jtj(JA, JB, absolute=False):
    """JA^T JB [7][7]: entry (a, b) = the sum over the rows r = 0..6 in that order, starting from the r = 0 product"""
    if absolute:
        JA, JB = np.abs(JA), np.abs(JB)
    s = JA[0][:, None] * JB[0][None, :]
    for r in range(1, 7):
        s = s + JA[r][:, None] * JB[r][None, :]
    return s


def _jte(J, e, absolute=False):
    if absolute:
        J, e = np.abs(J), np.abs(e)
    s = J[0] * e[0]
    for r in range(1, 7):
        s = s + J[r] * e[r]
    return s


def replay(P, J, E, mutant=None, stats=False):
    """H [7 nf][7 nf] and b [7 nf] in hessian order from the edges' Jacobians J [ne][2][7][7] and residuals E [ne][7]: plain Python
    over the edges in edge order, from v0, v1 and `fixed` alone.  For each edge the diagonal blocks J0^T J0 and J1^T J1 of its free
    ends, the block below the diagonal of a free pair -- J0^T J1 when vertex 0 has the higher hessian index, J1^T J0 otherwise -- and
    -J^T e, every product summed over the rows in order and added into H and b, which start from +0.0.  The upper triangle is the
    transpose of the lower one.  These are the device's float64 operations in the device's order, so the result is the device's bit
    for bit.
    mutant "exchanged": the two blocks below the diagonal take each other's place; "kind3": the J1^T J0 block is formed as J0^T J1
    (the exchange of the Jacobians forgotten).  stats: also the number of products and the sum of their magnitudes per entry."""
    h = hessian_index(P)
    nf = int((h >= 0).sum())
    H, b = np.zeros((7 * nf, 7 * nf)), np.zeros(7 * nf)
    nH, aH, nb, ab = np.zeros_like(H), np.zeros_like(H), np.zeros_like(b), np.zeros_like(b)
    for e in range(len(P["v0"])):
        hh = (int(h[P["v0"][e]]), int(h[P["v1"][e]]))
        for side in (0, 1):
            if hh[side] < 0:
                continue
            s = slice(7 * hh[side], 7 * hh[side] + 7)
            H[s, s] += _jtj(J[e, side], J[e, side])
            b[s] -= _jte(J[e, side], E[e])
            if stats:
                nH[s, s] += 7
                aH[s, s] += _jtj(J[e, side], J[e, side], True)
                nb[s] += 7
                ab[s] += _jte(J[e, side], E[e], True)
        if hh[0] >= 0 and hh[1] >= 0:
            first = hh[0] > hh[1]   # J0^T J1
            if mutant == "exchanged":
                first = not first
            elif mutant == "kind3":
                first = True
            hi, lo = max(hh), min(hh)
            JA, JB = (J[e, 0], J[e, 1]) if first else (J[e, 1], J[e, 0])
            H[7 * hi:7 * hi + 7, 7 * lo:7 * lo + 7] += _jtj(JA, JB)
            if stats:
                nH[7 * hi:7 * hi + 7, 7 * lo:7 * lo + 7] += 7
                aH[7 * hi:7 * hi + 7, 7 * lo:7 * lo + 7] += _jtj(JA, JB, True)
    low = np.tril(np.ones((nf, nf), bool), -1).repeat(7, axis=0).repeat(7, axis=1)
    H = np.where(low.T, H.T, H)
    if stats:
        return H, b, np.where(low.T, nH.T, nH), np.where(low.T, aH.T, aH), nb, ab
    return H, b


def pattern(P):
    """the entries of H [7 nf][7 nf] that an edge adds to"""
    h = hessian_index(P)
    nf = int((h >= 0).sum())
    blk = np.eye(nf, dtype=bool)
    a, b = h[P["v0"]], h[P["v1"]]
    both = (a >= 0) & (b >= 0)
    blk[a[both], b[both]] = blk[b[both], a[both]] = True
    return blk.repeat(7, axis=0).repeat(7, axis=1)


# ---------------------------------------------------------------------------------------------- a measurement that is not a number
def with_nan(P):
    """P with a NaN in one measurement: the linearisation has no finite chi2, no solve succeeds and no trial is accepted"""
    Sji = np.array(P["Sji"])
    Sji[len(Sji) // 2, 5] = np.nan
    return dict(P, Sji=Sji)
