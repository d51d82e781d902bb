"""What the OptimizeSim3 step tests share (tests/test_sim3_opt_steps_cpu.py on aos2_debug_sim3_opt_steps_host,
tests/test_sim3_opt_steps_gpu.py on aos2_debug_sim3_opt_steps_device): the cases, the items a case is run as (masks of planted act /
chi / outlier), the references in long double, the bounds, the comparisons, a replay of the device's sum and of the per-edge terms
that can be told to be wrong in three ways, and the write-down to profiles/sim3_opt_taps.txt.

Sizes: n in NS gives 2n = 2, 18, 64, 66, 254, 256, 258, 600 edges against the 256 threads of the workgroup and the 64 lanes of a wave:
most threads idle, exactly one wave, one pair into the next wave, one pair short of a stride, exactly one stride, one pair into the
second stride, three ragged strides.

The bounds.  b_J = 20 M DBL_EPSILON / (2 delta) on an entry of the Jacobian and b_E = 20 M DBL_EPSILON / 2 on a residual are those of
test_central_difference_jacobian_agrees_with_the_closed_form (tests/test_sim3_opt_cpu.py), M = the largest |pixel coordinate| among
the observations and the projections of the case.  Propagated to first order through what an edge adds (e' = e + de, J' = J + dJ,
|de_i| <= b_E, |dJ_ir| <= b_J; w the information, delta_H Huber's delta):
  chi2 = w (e_0^2 + e_1^2):          |d chi2| <= w (2 |e|_1 b_E + 2 b_E^2)                                            =: b_chi
  rho0, rho1 (chi2 <= delta_H^2):    rho0 = chi2, rho1 = 1:                 |d rho0| <= b_chi,       d rho1 = 0
             (chi2 >  delta_H^2):    rho0 = 2 sqrt(chi2) delta_H - delta_H^2, rho1 = delta_H / sqrt(chi2):
                                     |d rho0| <= rho1 b_chi,  |d rho1| <= rho1 b_chi / (2 chi2)
  H_rc = rho1 w sum_i J_ir J_ic:     |d H_rc| <= |d rho1| w sum_i |J_ir J_ic| + rho1 w sum_i (b_J (|J_ir| + |J_ic|) + b_J^2)
  b_r = -rho1 w sum_i J_ir e_i:      |d b_r|  <= |d rho1| w sum_i |J_ir e_i| + rho1 w sum_i (b_J |e_i| + b_E |J_ir| + b_J b_E)
First order in d rho1; the products of two entries are expanded in full, (J + dJ)(J + dJ) - J J = J dJ + dJ J + dJ dJ, because the
first-order part alone is no bound where it vanishes: the scale moves no projection of an e12 (x / z does not change with sigma), its
closed-form column 6 is 0 and its H_66 is the square of the central difference's rounding, at most 2 rho1 w b_J^2.
(every case keeps each chi2 a relative R.MARGIN from delta_H^2, so both sides take the same branch).  A sum of m terms in any order:
m 2^-53 sum |term| on top of the terms' own bounds."""
import os

import numpy as np

import sim3_opt_ref as R
from test_wave_sums_gpu import tree

DBL_EPSILON = 2.0 ** -52
LD = np.longdouble
NS = (1, 9, 32, 33, 127, 128, 129, 300)
SINGLES = (1, 9, 33)           # the sizes whose 2n single-edge masks are run
THREADS = 256                  # kSoThreads: edge e belongs to thread e % 256
LIN, TRIAL, REJECT = 1, 2, 4   # AOS2_SIM3_OPT_STEP_*
SEED = 11
UPDATE = (0.004, -0.003, 0.002, 0.01, -0.02, 0.015, 0.005)   # S_trial = exp(UPDATE) S_lin
SENTINEL, TAIL_BYTE = 0x5A, 0xA5
FIX_ZERO = (6, 12, 17, 21, 24, 26, 27, 34)   # the slots of Hb that column 6 of J feeds
IU = np.triu_indices(7)
CU = tuple(np.array([(r, c) for c in range(7) for r in range(c + 1)]).T)   # the upper triangle column by column
PAIRS = ((62, 63), (64, 65), (254, 255), (256, 257))   # edges on both sides of a wave's and of a stride's end


def sim3(S, dtype):
    return np.asarray(S[0], np.float64).astype(dtype), np.asarray(S[1], np.float64).astype(dtype), dtype(np.float64(S[2]))


def flat(S):
    return np.concatenate([np.asarray(S[0], np.float64), np.asarray(S[1], np.float64), [np.float64(S[2])]])


def interleave(a12, a21):
    """[n][...] of the e12 and of the e21 -> [2n][...] in edge order"""
    return np.stack([a12, a21], axis=1).reshape((2 * len(a12),) + a12.shape[1:])


def huber(chi, delta_h):
    big = chi > delta_h * delta_h
    sq = np.sqrt(np.where(big, chi, chi.dtype.type(1)))
    return big, np.where(big, 2 * sq * delta_h - delta_h * delta_h, chi), np.where(big, delta_h / sq, chi.dtype.type(1))


def edge_values(G, S):
    """residuals [2n][2], information [2n], chi2 [2n], rho0 [2n], rho1 [2n], above delta_H^2 [2n] in G's arithmetic"""
    e = interleave(*G.residuals(S))
    w = interleave(G.w1, G.w2)
    chi = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
    big, rho0, rho1 = huber(chi, G.huber)
    return e, w, chi, rho0, rho1, big


def terms_of(J, e, w, rho0, rho1, by_columns=False):
    """what constructQuadraticForm adds per edge [m][36]: H's upper triangle row by row (by_columns: the same entries column by
    column, which is wrong), b, rho0"""
    H = np.einsum("nir,n,nic->nrc", J, rho1 * w, J)
    H = H[:, CU[0], CU[1]] if by_columns else H[:, IU[0], IU[1]]
    b = np.einsum("nir,ni->nr", J, -(w[:, None] * e) * rho1[:, None])
    return np.concatenate([H, b, rho0[:, None]], axis=1)


def perturbed(S, fix_scale):
    """the 28 transforms of one linearisation in S's arithmetic: [2k] = exp(+-delta e_d) S (k = 2d: +, 2d + 1: -), [2k + 1] its inverse"""
    T = S[0].dtype.type
    out = []
    for k in range(14):
        add = np.zeros(7, S[0].dtype)
        add[k >> 1] = -T(R.DELTA) if k & 1 else T(R.DELTA)
        fwd = R.oplus(add, fix_scale, S)
        out += [fwd, R.sim3_inverse(fwd)]
    return out


def replay_terms(G, S, fix_scale, mutant=None):
    """the per-edge terms [2n][36] from the 28 perturbed transforms, as csrc/sim3_opt.h forms them, in G's arithmetic.  Without a
    mutant this is G.edge_terms.  mutant "forward": the e21 edges are differenced with the forward transforms, not the inverse ones;
    "columns": the triangle is filled column by column"""
    pert = perturbed(S, fix_scale)
    scalar = G.T(1) / (2 * G.delta)
    J12, J21 = np.zeros((G.n, 2, 7), G.dtype), np.zeros((G.n, 2, 7), G.dtype)
    for d in range(7):
        res12 = [G._res(G.o1, G.K1, R.sim3_map(pert[2 * k], G.X2)) for k in (2 * d, 2 * d + 1)]
        res21 = [G._res(G.o2, G.K2, R.sim3_map(pert[2 * k + (0 if mutant == "forward" else 1)], G.X1)) for k in (2 * d, 2 * d + 1)]
        J12[:, :, d], J21[:, :, d] = scalar * (res12[0] - res12[1]), scalar * (res21[0] - res21[1])
    e, w, chi, rho0, rho1, _ = edge_values(G, S)
    return terms_of(interleave(J12, J21), e, w, rho0, rho1, by_columns=mutant == "columns")


def block_sum(terms, act, skip_row=None):
    """SoDevEdges::block_sum over the active rows of terms [2n][K], in float64 two-operand additions: a running sum per thread over
    e = tid, tid + 256, ... starting from 0, the tree of row_sum_f64 over each row of 16 threads, the 16 row partials in row order.
    skip_row: that row of 16 lanes is left out (which is wrong)"""
    terms = np.asarray(terms, np.float64)
    per_thread = np.zeros((THREADS, terms.shape[1]))
    for e in range(len(terms)):
        if act[e]:
            per_thread[e % THREADS] = per_thread[e % THREADS] + terms[e]
    part = tree(per_thread.reshape(THREADS // 16, 16, -1))
    total = None
    for r in range(THREADS // 16):
        if r == skip_row:
            continue
        total = part[r] if total is None else total + part[r]
    return total


# ---------------------------------------------------------------------------------------------- the cases
def _case(n, fix, far, rng):
    n_out = 1 if n == 1 else max(2, n // 5)
    if n == 1 and fix:
        n_out = 0
    P = R.problem(rng, n, n_out, fix, far)
    S_lin = (np.asarray(P["q12"], np.float64), np.asarray(P["t12"], np.float64), np.float64(P["s12"]))
    S_trial = R.oplus(np.array(UPDATE), fix, S_lin)
    G = R.Graph(P, np.float64)
    d2 = G.huber * G.huber
    chis = np.concatenate([edge_values(G, S)[2] for S in (S_lin, S_trial)])
    margin = float(np.abs(chis - d2).min() / d2)
    return dict(name="n%d_fix%d_%s" % (n, fix, "far" if far else "near"), P=P, n=n, fix=fix, far=far, S_lin=S_lin, S_trial=S_trial, margin=margin,
                n_above=int((chis[:2 * n] > d2).sum()))


_CASES = {}


def cases():
    """name -> case, in a fixed order; "dropped" / "drawn" count the candidates that came within R.MARGIN of delta_H^2"""
    if not _CASES:
        dropped = drawn = 0
        out = {}
        for i, n in enumerate(NS):
            for fix in (False, True):
                far = bool((i + fix) % 2)
                for j in range(16):
                    drawn += 1
                    c = _case(n, fix, far, np.random.default_rng([SEED, n, fix, j]))
                    if c["margin"] >= R.MARGIN:
                        break
                    dropped += 1
                else:
                    raise RuntimeError("no candidate of n = %d keeps the margin" % n)
                c["masks"] = _masks(c)
                out[c["name"]] = c
        _CASES.update(cases=out, dropped=dropped, drawn=drawn)
    return _CASES["cases"]


def draw_counts():
    cases()
    return _CASES["dropped"], _CASES["drawn"]


def _masks(c):
    """name -> act [2n] (uint8).  Pair-consistent but for the single-edge masks"""
    n = c["n"]
    rng = np.random.default_rng([SEED, n, 77])
    half = rng.random(n) < 0.5
    if n > 1:
        half[0], half[n - 1] = True, False
    column = np.arange(n) % (THREADS // 2) != (n - 1) % (THREADS // 2)   # threads 2 col and 2 col + 1 own nothing that is active
    m = dict(all=np.ones(n, bool), half=half, column=column, none=np.zeros(n, bool))
    return {k: np.repeat(v, 2).astype(np.uint8) for k, v in m.items()}


def chi_planted(c):
    """chi_in of the linearise / trial items: values no chi2 of the case equals"""
    return np.random.default_rng([SEED, c["n"], 5]).uniform(100.0, 200.0, 2 * c["n"])


def step_items(c):
    """[(tag, item)] of one case: the four masks with S_trial = exp(UPDATE) S_lin, and `all` and `half` again with S_trial = S_lin"""
    chi_in, zero = chi_planted(c), np.zeros(c["n"], np.uint8)
    items = []
    for tag, same in (("all", False), ("half", False), ("column", False), ("none", False), ("all", True), ("half", True)):
        items.append((tag + ("_same" if same else ""), dict(problem=c["P"], S_lin=c["S_lin"], S_trial=c["S_lin"] if same else c["S_trial"],
                                                            act_in=c["masks"][tag], chi_in=chi_in, outlier_in=zero, remove=0, mask=LIN | TRIAL)))
    return items


def single_items(c):
    """the 2n single-edge masks of a case of SINGLES"""
    chi_in, zero = chi_planted(c), np.zeros(c["n"], np.uint8)
    eye = np.eye(2 * c["n"], dtype=np.uint8)
    return [dict(problem=c["P"], S_lin=c["S_lin"], S_trial=c["S_trial"], act_in=eye[e], chi_in=chi_in, outlier_in=zero, remove=0, mask=LIN | TRIAL)
            for e in range(2 * c["n"])]


def batches(items, size=64):
    return [items[k:k + size] for k in range(0, len(items), size)]


# ---------------------------------------------------------------------------------------------- references and bounds
_REF = {}


def reference(c):
    """the long double side of a case, once per process: the perturbed transforms and their measured bound; at S_lin the residuals,
    the closed-form Jacobian, the per-edge terms formed from them and from long double central differences, the propagated bounds;
    at S_trial chi2, rho0 and their bounds.  The references stay long double; the bounds are formed in float64."""
    if c["name"] in _REF:
        return _REF[c["name"]]
    P, fix = c["P"], c["fix"]
    G, G64 = R.Graph(P, LD), R.Graph(P, np.float64)
    S_lin, S_trial = sim3(c["S_lin"], LD), sim3(c["S_trial"], LD)
    # the transforms: 4 x the largest difference of the restatement between float64 and long double, floor 8 DBL_EPSILON max(1, |S_lin|)
    pert = np.stack([np.concatenate([q, t, [s]]) for q, t, s in perturbed(S_lin, fix)])
    pert64 = np.stack([flat(T) for T in perturbed(sim3(c["S_lin"], np.float64), fix)])
    measured = float(np.abs(pert64.astype(LD) - pert).max())
    floor = 8 * DBL_EPSILON * max(1.0, float(np.abs(flat(c["S_lin"])).max()))
    out = dict(pert=pert, pert_measured=measured, pert_floor=floor, pert_bound=max(floor, 4 * measured))
    # M, b_J, b_E
    M = 0.0
    for S in (c["S_lin"], c["S_trial"]):
        e12, e21 = G64.residuals(S)
        M = max(M, np.abs(G64.o1).max(), np.abs(G64.o2).max(), np.abs(G64.o1 - e12).max(), np.abs(G64.o2 - e21).max())
    b_J, b_E = 20 * M * DBL_EPSILON / (2 * R.DELTA), 20 * M * DBL_EPSILON / 2
    out.update(M=float(M), b_J=b_J, b_E=b_E)

    def bounds(e, w, chi, rho1, big):
        b_chi = w * (2 * np.abs(e).sum(axis=1) * b_E + 2 * b_E * b_E)
        return b_chi, np.where(big, rho1, 1.0) * b_chi, np.where(big, rho1 * b_chi / (2 * chi), 0.0)

    # S_lin
    e, w, chi, rho0, rho1, big = edge_values(G, S_lin)
    J = interleave(*R.closed_form_jacobians(G, S_lin))
    if fix:
        J[:, :, 6] = 0
    terms, chi_ld = terms_of(J, e, w, rho0, rho1), chi
    e, w, chi, rho0, rho1, J = (np.asarray(a, np.float64) for a in (e, w, chi, rho0, rho1, J))
    b_chi, b_rho0, b_rho1 = bounds(e, w, chi, rho1, big)
    aJ, ae = np.abs(J), np.abs(e)
    col = aJ.sum(axis=1)   # [2n][7]: sum_i |J_ir|
    bH = (b_rho1 * w)[:, None, None] * np.einsum("nir,nic->nrc", aJ, aJ) + (rho1 * w)[:, None, None] * (b_J * (col[:, :, None] + col[:, None, :]) + 2 * b_J * b_J)
    bb = b_rho1[:, None] * w[:, None] * np.einsum("nir,ni->nr", aJ, ae) + (rho1 * w)[:, None] * (b_J * ae.sum(axis=1)[:, None] + b_E * col + 2 * b_J * b_E)
    out.update(terms=terms, terms_bound=np.concatenate([bH[:, IU[0], IU[1]], bb, b_rho0[:, None]], axis=1), chi_lin=chi_ld, b_chi_lin=b_chi,
               terms_cd=G.edge_terms(S_lin, fix), above=big)
    # S_trial
    e, w, chi_ld, rho0_ld, rho1, big = edge_values(G, S_trial)
    b_chi, b_rho0, _ = bounds(np.asarray(e, np.float64), np.asarray(w, np.float64), np.asarray(chi_ld, np.float64), np.asarray(rho1, np.float64), big)
    out.update(chi_trial=chi_ld, b_chi_trial=b_chi, rho0_trial=rho0_ld, b_rho0_trial=b_rho0)
    _REF[c["name"]] = out
    return out


def worst(diff, bound):
    """the largest diff / bound; a difference where the bound is 0 counts as infinite"""
    diff, bound = np.broadcast_arrays(np.asarray(diff, np.float64), np.asarray(bound, np.float64))
    if diff.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max())


def bits(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype).tobytes()


# ---------------------------------------------------------------------------------------------- the comparisons (each -> a ratio, <= 1 passes)
def ratio_pert(c, got_pert):
    """the 28 transforms against the long double ones"""
    ref = reference(c)
    return worst(np.abs(np.asarray(got_pert, np.float64).astype(LD) - ref["pert"]), ref["pert_bound"])


def fix_scale_exact(c, out):
    """with a fixed scale: the two perturbations of the scale are the same transform, and column 6 of J feeds exact zeros"""
    if not c["fix"]:
        return True
    p, Hb = out["pert"], out["Hb"]
    return bits(p[24]) == bits(p[26]) and bits(p[25]) == bits(p[27]) and all(Hb[k] == 0 for k in FIX_ZERO)


def ratio_single(c, e, Hb):
    """Hb of the item whose only active edge is e against that edge's terms from the closed-form Jacobian"""
    ref = reference(c)
    return worst(np.abs(np.asarray(Hb, np.float64).astype(LD) - ref["terms"][e]), ref["terms_bound"][e])


def ratio_sum(c, act, Hb):
    """Hb against the long double sum of the reference's per-edge terms over the active edges, any order"""
    ref, a = reference(c), np.asarray(act, bool)
    t = ref["terms_cd"][a]
    bound = a.sum() * 2.0 ** -53 * np.abs(t).sum(axis=0).astype(np.float64) + ref["terms_bound"][a].sum(axis=0)
    return worst(np.abs(np.asarray(Hb, np.float64).astype(LD) - t.sum(axis=0)), bound)


def ratio_chi(c, act, chi_in, got, which):
    """chi [2n] after linearise (which = "lin") or after trial ("trial"): active edges against the long double chi2, inactive edges
    keep chi_in byte for byte (-> inf otherwise)"""
    ref, a = reference(c), np.asarray(act, bool)
    got = np.asarray(got, np.float64)
    if bits(got[~a]) != bits(np.asarray(chi_in)[~a]):
        return np.inf
    return worst(np.abs(got[a] - ref["chi_" + which][a]), ref["b_chi_" + which][a])


def ratio_trial_sum(c, act, got):
    ref, a = reference(c), np.asarray(act, bool)
    r = ref["rho0_trial"][a]
    bound = a.sum() * 2.0 ** -53 * float(np.abs(r).sum()) + ref["b_rho0_trial"][a].sum()
    return worst(abs(LD(np.asarray(got, np.float64).reshape(-1)[0]) - r.sum()), bound)


def untouched(out, names):
    """the buffers `names` still hold the sentinel in every byte"""
    return all((np.asarray(out[k]).view(np.uint8) == SENTINEL).all() for k in names)


def tails_kept(out, n):
    """what lies behind act / chi / outlier came back as it went in"""
    return all((np.asarray(out[k][m:]).view(np.uint8) == TAIL_BYTE).all() and len(out[k][m:]) > 0 for k, m in (("act", 2 * n), ("chi", 2 * n), ("outlier", n)))


def graph_outputs(c, act, same, dtype=np.float64, mutant=None):
    """what an item gives when the restatement R.Graph runs it in `dtype`, sums in edge order: Hb, pert, chi_lin, trial_sum, chi_trial
    (chi of inactive edges from chi_planted).  mutant: replay_terms' or "row" (block_sum without row 1)"""
    G = R.Graph(c["P"], dtype)
    S_lin = sim3(c["S_lin"], dtype)
    S_trial = S_lin if same else sim3(c["S_trial"], dtype)
    a, chi_in = np.asarray(act, bool), chi_planted(c)
    terms = replay_terms(G, S_lin, c["fix"], mutant) if mutant in ("forward", "columns") else G.edge_terms(S_lin, c["fix"])
    if mutant == "row":
        Hb = block_sum(terms, a, skip_row=1)
    else:
        Hb = np.zeros(36, dtype)
        for row in terms[a]:
            Hb = Hb + row
    _, _, chi_l, _, _, _ = edge_values(G, S_lin)
    _, _, chi_t, rho0_t, _, _ = edge_values(G, S_trial)
    total = dtype(0)
    for r in rho0_t[a]:
        total = total + r
    return dict(Hb=np.asarray(Hb, np.float64), pert=np.stack([flat(T) for T in perturbed(S_lin, c["fix"])]), terms=terms,
                chi_lin=np.where(a, np.asarray(chi_l, np.float64), chi_in), trial_sum=np.float64(total),
                chi_trial=np.where(a, np.asarray(chi_t, np.float64), chi_in))


# ---------------------------------------------------------------------------------------------- reject on planted chi
def reject_item(c, remove):
    """chi, act and outlier planted for reject alone -> (item, expected dict).  Correspondences 0..7 (n >= 9) take one kind each: below
    th2, above in both, above in the e12 only, above in the e21 only, exactly th2, NaN, an inactive pair holding 1e300, below with
    outlier_in = 1; the rest take kinds at random.  The pairs of PAIRS and the last pair of the case are flagged (a different kind each)."""
    n = c["n"]
    rng = np.random.default_rng([SEED, n, int(c["fix"]), int(remove), 9])
    th2 = float(np.float32(c["P"]["th2"]))
    kind = rng.integers(0, 8, n)
    if n >= 9:
        kind[:8] = np.arange(8)
    forced = [e0 // 2 for e0, _ in PAIRS if e0 // 2 < n] + [n - 1]
    for j, k in enumerate(forced):
        kind[k] = (1, 2, 3)[(j + n) % 3]
    chi = rng.uniform(0.0, 0.999 * th2, (n, 2))
    hi = lambda m: rng.uniform(1.001 * th2, 50 * th2, m)   # noqa: E731
    act, out_in = np.ones(n, np.uint8), (rng.random(n) < 0.15).astype(np.uint8)
    for k in range(n):
        if kind[k] == 1:
            chi[k] = hi(2)
        elif kind[k] == 2:
            chi[k, 0] = hi(1)[0]
        elif kind[k] == 3:
            chi[k, 1] = hi(1)[0]
        elif kind[k] == 4:
            chi[k] = th2
        elif kind[k] == 5:
            chi[k, rng.integers(0, 2)] = np.nan
        elif kind[k] == 6:
            chi[k], act[k] = 1e300, 0
        elif kind[k] == 7:
            out_in[k] = 1
    bad = (act != 0) & ((chi[:, 0] > th2) | (chi[:, 1] > th2))
    act2 = np.repeat(act, 2)
    item = dict(problem=c["P"], S_lin=c["S_lin"], S_trial=c["S_trial"], act_in=act2, chi_in=chi.reshape(-1), outlier_in=out_in, remove=int(remove), mask=REJECT)
    want = dict(flagged=int(bad.sum()), outlier=out_in | bad.astype(np.uint8), act=np.where(np.repeat(bad, 2) & bool(remove), 0, act2).astype(np.uint8),
                chi=chi.reshape(-1), kinds=set(kind.tolist()), bad=bad)
    return item, want


def reject_failures(c, item, want, out):
    """what of reject's contract `out` does not meet (an empty list passes)"""
    n, fails = c["n"], []
    if int(out["flagged"][0]) != want["flagged"]:
        fails.append("count %d, expected %d" % (out["flagged"][0], want["flagged"]))
    if not np.array_equal(out["outlier"][:n], want["outlier"]):
        fails.append("outlier differs at %s" % np.flatnonzero(out["outlier"][:n] != want["outlier"])[:8])
    if not np.array_equal(out["act"][:2 * n], want["act"]):
        fails.append("act differs at %s" % np.flatnonzero(out["act"][:2 * n] != want["act"])[:8])
    if bits(out["chi"][:2 * n]) != bits(want["chi"]):
        fails.append("chi was touched")
    if not tails_kept(out, n):
        fails.append("a byte behind 2n / n changed")
    if not untouched(out, ("Hb", "pert", "chi_lin", "trial_sum", "chi_trial")):
        fails.append("a step that was not asked for wrote")
    return fails


# ---------------------------------------------------------------------------------------------- the write-down
TAPS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sim3_opt_taps.txt")
TAPS_HEAD = ["# OptimizeSim3: the step taps against their references (tests/test_sim3_opt_steps_cpu.py: `reference`, the float64 restatement and",
             "# what the bounds are made of, and `host`, aos2_debug_sim3_opt_steps_host; tests/test_sim3_opt_steps_gpu.py: `device`,",
             "# aos2_debug_sim3_opt_steps_device), one line per case: the worst difference / bound of every comparison (<= 1 passes);",
             "# comparisons that are bit for bit are named as such"]


def record(key, text):
    """keep `key: text` in profiles/sim3_opt_taps.txt (the other lines stay)"""
    lines = {}
    if os.path.exists(TAPS_FILE):
        with open(TAPS_FILE) as f:
            for ln in f.read().splitlines():
                if ln and not ln.startswith("#") and ": " in ln:
                    lines[ln.split(": ", 1)[0]] = ln.split(": ", 1)[1]
    lines[key] = text
    with open(TAPS_FILE, "w") as f:
        f.write("\n".join(TAPS_HEAD + ["%s: %s" % kv for kv in sorted(lines.items())]) + "\n")
