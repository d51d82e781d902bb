"""Frame::ComputeStereoMatches (reference src/Frame.cc:495-669) restated in plain numpy from the reference's text, with a
trace that says why every left keypoint ended as it did, the domain rule of include/aos2.h, and the planted worlds the
stereo tests run on.

Every `float` of the reference is an np.float32 scalar here and every operation on them is written out in the reference's
order, so the results are meant to agree bit for bit.  Where the reference leaves the behaviour open this module says so:

* :521  vRowIndices[yi] is indexed without a guard; a band that leaves the image writes outside the vector.  Here the band
        is cut at row 0 and at the last row (only keypoints within 2 * scale of the border get there).
* :592, :609  rowRange / colRange throw when a window leaves the plane.  Here that is a ValueError: callers stay inside
        in_domain(), the same rule the host-pointer entry of the library enforces.
* :633  `deltaR < -1 || deltaR > 1` cannot fire.  dist2 is the FIRST strict minimum and sits at an interior offset, so
        dist1 > dist2 and dist3 >= dist2: the denominator 2 (dist1 + dist3 - 2 dist2) is positive and |dist1 - dist3| <=
        (dist1 - dist2) + (dist3 - dist2), hence |deltaR| <= 0.5.  All sums are integers below 2^24, so float changes
        nothing.  compute() asserts it for every keypoint that reaches the line.
* :646  `bestuR = uL-0.01` is formed in double and rounded to float once; :645 assigns the double 0.01 to a float.
* :656  vDistIdx[0] of an empty vector is read when nothing matched.  Here nothing is culled and the median is None.
"""
import numpy as np

F = np.float32
TH_HIGH, TH_LOW = 100, 50                     # src/ORBmatcher.cc:37-38
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

REASONS = ("NO_CANDIDATES", "NO_DESCRIPTOR_MATCH", "WINDOW_OUT", "BEST_AT_END", "DISPARITY_OUT", "ACCEPTED",
           "ACCEPTED_ZERO_DISPARITY", "CULLED")
(NO_CANDIDATES, NO_DESCRIPTOR_MATCH, WINDOW_OUT, BEST_AT_END, DISPARITY_OUT, ACCEPTED, ACCEPTED_ZERO_DISPARITY,
 CULLED) = range(8)

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _round(v):
    """::round(float): halves go away from zero"""
    v = float(v)
    return F(np.copysign(np.floor(abs(v) + 0.5), v))


def _window(plane, cv, cu, what):
    """plane.rowRange(cv-5, cv+6).colRange(cu-5, cu+6) as CV_32F"""
    h, w = plane.shape
    if cv - 5 < 0 or cv + 6 > h or cu - 5 < 0 or cu + 6 > w:
        raise ValueError(f"{what}: window at ({cu}, {cv}) leaves the {w} x {h} plane (cv::Exception in the reference)")
    return plane[cv - 5:cv + 6, cu - 5:cu + 6].astype(F)


def compute(kl, dl, kr, dr, mb, mbf, scale, inv_scale, planes_l, planes_r):
    """-> (mvuRight, mvDepth, trace).  planes_*[level] = mvImagePyramid[level] of each eye (2-D uint8 arrays)."""
    N, Nr = len(kl), len(kr)
    mb, mbf = F(mb), F(mbf)
    scale, inv_scale = np.asarray(scale, F), np.asarray(inv_scale, F)
    u_right, depth = np.full(N, -1.0, F), np.full(N, -1.0, F)                                   # :497-498
    tr = dict(reason=np.full(N, NO_CANDIDATES, np.int8), best_idx=np.full(N, -1, np.int64),
              hamming=np.full(N, TH_HIGH, np.int64), sums=np.full((N, 11), -1, np.int64),
              best_inc=np.zeros(N, np.int64), delta=np.full(N, np.nan, F), best_sum=np.full(N, -1, np.int64),
              median=None, th_dist=None, n_before_cull=0)
    th_orb = (TH_HIGH + TH_LOW) // 2                                                            # :500
    n_rows = planes_l[0].shape[0]                                                               # :502
    rows = [[] for _ in range(n_rows)]
    for iR in range(Nr):                                                                        # :512-522
        kpY = F(kr["y"][iR])
        r = F(2.0) * scale[kr["octave"][iR]]
        maxr, minr = int(np.ceil(kpY + r)), int(np.floor(kpY - r))
        for yi in range(max(minr, 0), min(maxr, n_rows - 1) + 1):
            rows[yi].append(iR)
    minZ, minD = mb, F(0)                                                                       # :525-527
    maxD = mbf / minZ
    xr_all, oct_r = kr["x"].astype(F), kr["octave"]
    dist_idx = []
    for iL in range(N):
        levelL, vL, uL = int(kl["octave"][iL]), F(kl["y"][iL]), F(kl["x"][iL])
        row = int(vL)                                                                           # :540, float -> size_t
        if not 0 <= row < n_rows:
            raise ValueError(f"left keypoint {iL}: row {row} outside vRowIndices")
        cand = rows[row]
        if not cand:
            continue
        minU, maxU = uL - maxD, uL - minD
        if maxU < 0:
            continue
        bestDist, bestIdxR = TH_HIGH, 0
        for iR in cand:                                                                         # :557-578
            if oct_r[iR] < levelL - 1 or oct_r[iR] > levelL + 1:
                continue
            uR = xr_all[iR]
            if uR >= minU and uR <= maxU:
                dist = int(_POP[dl[iL] ^ dr[iR]].sum())
                if dist < bestDist:
                    bestDist, bestIdxR = dist, iR
        tr["hamming"][iL] = bestDist
        if not bestDist < th_orb:                                                               # :581
            tr["reason"][iL] = NO_DESCRIPTOR_MATCH
            continue
        tr["best_idx"][iL] = bestIdxR
        uR0 = xr_all[bestIdxR]
        scaleFactor = inv_scale[levelL]
        scaleduL, scaledvL, scaleduR0 = _round(uL * scaleFactor), _round(vL * scaleFactor), _round(uR0 * scaleFactor)
        PL, PR = planes_l[levelL], planes_r[levelL]
        IL = _window(PL, int(scaledvL), int(scaleduL), f"left keypoint {iL}")                    # :592-594
        IL = IL - IL[5, 5]
        iniu = scaleduR0 + F(5) - F(5)                                                          # :602-605
        endu = scaleduR0 + F(5) + F(5) + F(1)
        if iniu < 0 or endu >= PR.shape[1]:
            tr["reason"][iL] = WINDOW_OUT
            continue
        bestS, bestincR = 2 ** 31 - 1, 0
        vDists = np.zeros(11, F)
        for incR in range(-5, 6):                                                               # :607-621
            IR = _window(PR, int(scaledvL), int(scaleduR0) + incR, f"right window of left keypoint {iL}")
            IR = IR - IR[5, 5]
            dist = F(np.abs(IL - IR).sum(dtype=np.float64))   # cv::norm(NORM_L1) of CV_32F sums in double
            if dist < F(bestS):
                bestS, bestincR = int(dist), incR
            vDists[5 + incR] = dist
        tr["sums"][iL] = vDists.astype(np.int64)
        tr["best_inc"][iL], tr["best_sum"][iL] = bestincR, bestS
        if bestincR == -5 or bestincR == 5:                                                     # :623
            tr["reason"][iL] = BEST_AT_END
            continue
        dist1, dist2, dist3 = vDists[5 + bestincR - 1], vDists[5 + bestincR], vDists[5 + bestincR + 1]
        deltaR = (dist1 - dist3) / (F(2.0) * (dist1 + dist3 - F(2.0) * dist2))                  # :631
        tr["delta"][iL] = deltaR
        assert dist1 > dist2 and dist3 >= dist2 and abs(deltaR) <= F(0.5), "the gate of :633 cannot fire"
        bestuR = scale[levelL] * (scaleduR0 + F(bestincR) + deltaR)                             # :637
        disparity = uL - bestuR
        if disparity >= minD and disparity < maxD:                                              # :641-651
            tr["reason"][iL] = ACCEPTED
            if disparity <= 0:
                disparity = F(0.01)
                bestuR = F(np.float64(uL) - 0.01)
                tr["reason"][iL] = ACCEPTED_ZERO_DISPARITY
            depth[iL] = mbf / disparity
            u_right[iL] = bestuR
            dist_idx.append((bestS, iL))
        else:
            tr["reason"][iL] = DISPARITY_OUT
    tr["n_before_cull"] = len(dist_idx)
    if dist_idx:
        dist_idx.sort()                                                                         # :655-668
        median = F(dist_idx[len(dist_idx) // 2][0])
        thDist = F(1.5) * F(1.4) * median
        tr["median"], tr["th_dist"] = median, thDist
        for first, second in reversed(dist_idx):
            if F(first) < thDist:
                break
            u_right[second] = depth[second] = F(-1)
            tr["reason"][second] = CULLED
    return u_right, depth, tr


def reason_counts(trace):
    return {name: int((trace["reason"] == i).sum()) for i, name in enumerate(REASONS)}


def in_domain(kl, kr, level_sizes, inv_scale):
    """The rule of include/aos2.h ("Domain of ComputeStereoMatches").  level_sizes[l] = (w, h).  -> (ok, why)"""
    nlevels, inv = len(level_sizes), np.asarray(inv_scale, F)
    rows = level_sizes[0][1]
    for i in range(len(kl)):
        o, x, y = int(kl["octave"][i]), F(kl["x"][i]), F(kl["y"][i])
        if not 0 <= o < nlevels or not np.isfinite(x) or not np.isfinite(y):
            return False, f"left {i}: octave or position"
        w, h = level_sizes[o]
        cu, cv = _round(x * inv[o]), _round(y * inv[o])
        if not -1 < y < rows or not 5 <= cv <= h - 6 or not 5 <= cu <= w - 6:
            return False, f"left {i}: window leaves level {o}"
    for i in range(len(kr)):
        o, x, y = int(kr["octave"][i]), F(kr["x"][i]), F(kr["y"][i])
        if not 0 <= o < nlevels or not np.isfinite(y):
            return False, f"right {i}: octave or y"
        for lv in range(max(o - 1, 0), min(o + 1, nlevels - 1) + 1):
            if 0 <= _round(x * inv[lv]) < 10:
                return False, f"right {i}: search window leaves level {lv}"
    return True, ""


# ---------------------------------------------------------------------------------------------------------------------
# Planted worlds.  A world is a uniform-noise pair (values <= 234) with right(x) = left(x + D), a few tiles written over
# it, and hand-built keypoint / descriptor arrays.  The extractors only run on the images so that the pyramids exist.
#
# At level 0 the scale is 1, so a left keypoint at integer (xL, y) and a right keypoint near xL - D read exactly the
# pixels the builder knows.  The aligned SAD of an unedited pair is 0; adding 1 to k non-centre pixels of the right
# window makes it exactly k, adding k to one pixel likewise (<= 234 + 21 = 255, nothing saturates).  The misaligned sums
# are about 10^4, so the aligned offset stays the first strict minimum.  Tiles of edited pairs are 22 px apart in x and
# 12 px in y: the 21 x 11 right windows are disjoint and the row bands (y +- 2 at octave 0) see only their own tile row.

D = 12          # disparity of the noise pairs
X0 = 46         # x of the first tile: its right keypoint (x = 34) is in the domain at every octave the worlds give it
NLEVELS, SCALE_FACTOR = 8, 1.2
SCALE = np.array([F(1.0)] * NLEVELS, F)
for _l in range(1, NLEVELS):                  # src/ORBextractor.cc:424-431
    SCALE[_l] = SCALE[_l - 1] * F(SCALE_FACTOR)
INV_SCALE = (F(1.0) / SCALE).astype(F)


def level_sizes(w, h):
    """(w, h) of every level, src/ORBextractor.cc:1112: cvRound(size * inv)"""
    return [(int(np.rint(F(w) * INV_SCALE[l])), int(np.rint(F(h) * INV_SCALE[l]))) for l in range(NLEVELS)]


class World:
    def __init__(self, name, w, h, seed, mb, mbf, nfeatures=500):
        self.name, self.w, self.h, self.mb, self.mbf, self.nfeatures = name, w, h, F(mb), F(mbf), nfeatures
        self.rng = np.random.default_rng(seed)
        self.left = self.rng.integers(0, 235, (h, w), dtype=np.uint8)
        self.right = self.rng.integers(0, 235, (h, w), dtype=np.uint8)
        self.right[:, :w - D] = self.left[:, D:]
        self._kl, self._dl, self._kr, self._dr = [], [], [], []
        self.tags, self.expect = [], []          # per left keypoint: what it was planted for, the reason it must end with
        self._next_row = 0
        self._tiles = None

    # -- geometry: tile (i, j) has its left keypoint at (X0 + 22 i, 8 + 12 j)
    def tile_rows(self):
        return (self.h - 6 - 8) // 12 + 1

    def tile_cols(self):
        return (self.w - 6 - X0) // 22 + 1

    def take_row(self):
        """the y of a tile row nothing else uses"""
        j = self._next_row
        self._next_row += 1
        assert j < self.tile_rows(), "no tile row left"
        return 8 + 12 * j

    def take_tile(self):
        if not self._tiles:
            y = self.take_row()
            self._tiles = [(X0 + 22 * i, y) for i in range(self.tile_cols())][::-1]
        return self._tiles.pop()

    def new_row(self):
        self._tiles = None

    # -- records
    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flipped(self, desc, nbits):
        bits = np.unpackbits(desc)
        bits[self.rng.choice(256, nbits, replace=False)] ^= 1
        return np.packbits(bits)

    def add_right(self, x, y, desc, octave=0):
        self._kr.append((x, y, octave))
        self._dr.append(desc)
        return len(self._kr) - 1

    def add_left(self, x, y, desc, tag, expect=None, octave=0):
        self._kl.append((x, y, octave))
        self._dl.append(desc)
        self.tags.append(tag)
        self.expect.append(expect)
        return len(self._kl) - 1

    # -- pixels
    def edit(self, xr, y, dx, dy, delta):
        assert (dx, dy) != (0, 0) and abs(dx) <= 5 and abs(dy) <= 5
        v = int(self.right[y + dy, xr + dx]) + delta
        assert v <= 255
        self.right[y + dy, xr + dx] = v

    def make_sum(self, xr, y, s, single=False, symmetric=False):
        """aligned SAD of the pair whose right window is centred at (xr, y) becomes exactly s"""
        if s == 0:
            return
        if single:
            k = int(self.rng.choice([i for i in range(121) if i != 60]))
            self.edit(xr, y, k % 11 - 5, k // 11 - 5, s)
        elif symmetric:                      # keeps a mirror-symmetric strip symmetric: pairs (dx, dy), (-dx, dy)
            assert s % 2 == 0
            cells = [(dx, dy) for dy in range(-5, 6) for dx in range(1, 6)]
            for c in self.rng.choice(len(cells), s // 2, replace=False):
                self.edit(xr, y, cells[c][0], cells[c][1], 1)
                self.edit(xr, y, -cells[c][0], cells[c][1], 1)
        else:
            for k in self.rng.choice([i for i in range(121) if i != 60], s, replace=False):
                self.edit(xr, y, int(k) % 11 - 5, int(k) // 11 - 5, 1)

    def tile(self, xl, xr, y, half_r=10, mirror=False):
        """one fresh random pattern centred at xl in the left image (11 wide) and at xr in the right one (2 half_r + 1 wide)"""
        half = max(half_r, 5)
        p = self.rng.integers(0, 235, (11, 2 * half + 1), dtype=np.uint8)
        if mirror:
            p[:, half + 1:] = p[:, :half][:, ::-1]
        self.left[y - 5:y + 6, xl - 5:xl + 6] = p[:, half - 5:half + 6]
        self.right[y - 5:y + 6, xr - half_r:xr + half_r + 1] = p[:, half - half_r:half + half_r + 1]

    def tile_periodic(self, xl, xr, y, period=3):
        """a right strip that repeats every `period` columns and the left patch cut from its middle: the sums at the offsets
        that are multiples of the period are all 0"""
        base = self.rng.integers(0, 235, (11, period), dtype=np.uint8)
        strip = base[:, (np.arange(21) - 10) % period]
        self.right[y - 5:y + 6, xr - 10:xr + 11] = strip
        self.left[y - 5:y + 6, xl - 5:xl + 6] = strip[:, 5:16]

    def pair(self, tag, s=0, ham=0, expect=ACCEPTED, single=False, kp_dx=0, at=None, octave_r=0, yr=None, left=True):
        """a left keypoint on a tile of the noise pair and its right partner kp_dx px beside the true place"""
        xl, y = at or self.take_tile()
        xr = xl - D
        self.make_sum(xr, y, s, single)
        d = self.desc()
        iR = self.add_right(F(xr + kp_dx), F(y if yr is None else yr), self.flipped(d, ham), octave_r)
        iL = self.add_left(F(xl), F(y), d, tag, expect) if left else None
        return iL, iR

    # -- result
    def arrays(self):
        def kps(rec):
            a = np.zeros(len(rec), KP_DTYPE)
            for i, (x, y, o) in enumerate(rec):
                a[i] = (x, y, F(31.0) * SCALE[o], 0.0, 1.0, o, -1)
            return a
        dl = np.array(self._dl, np.uint8).reshape(-1, 32)
        dr = np.array(self._dr, np.uint8).reshape(-1, 32)
        return kps(self._kl), dl, kps(self._kr), dr

    def sizes(self):
        return level_sizes(self.w, self.h)

    def which(self, tag):
        return [i for i, t in enumerate(self.tags) if t == tag or t.startswith(tag + ":")]


def _sums_world(name, sums, seed, singles=(), culled=()):
    W = World(name, 320, 240, seed, 0.5, 40.0)
    for i, s in enumerate(sums):
        W.pair(f"sum:{s}", s, single=(i in singles), expect=CULLED if s in culled else ACCEPTED)
        if i % 3 == 2:
            W.new_row()
    return W


def world_pixels():
    """every pixel of the 11 x 11 patch counts once: +21 on each non-centre pixel in turn is culled, +20 is kept, and 260
    pairs of sum 10 hold the median at 10 (thDist = 21)"""
    W = World("pixels", 640, 480, 11, 0.5, 40.0)
    specs = [("pix21", k) for k in range(121) if k != 60] + [("pix20", k) for k in range(121) if k != 60] + [("ten", None)] * 260
    order = np.random.default_rng(5).permutation(len(specs))
    for o in order:
        kind, k = specs[o]
        xl, y = W.take_tile()
        if kind == "ten":
            W.pair("ten", 10, at=(xl, y))
        else:
            delta = 21 if kind == "pix21" else 20
            W.edit(xl - D, y, k % 11 - 5, k // 11 - 5, delta)
            W.pair(f"{kind}:{k}", 0, at=(xl, y), expect=CULLED if delta == 21 else ACCEPTED)
    return W


def world_nomatch():
    """no left keypoint gets past the descriptor test: nothing to take a median of"""
    W = World("nomatch", 320, 240, 21, 0.5, 40.0)
    for _ in range(5):
        W.pair("far", 0, ham=128, expect=NO_DESCRIPTOR_MATCH)
    W.add_left(F(100), F(W.take_row()), W.desc(), "empty_row", NO_CANDIDATES)
    return W


def world_hamming():
    """the descriptor stage: thOrbDist from both sides, ties between right candidates, rows of 1 .. 129 candidates"""
    W = World("hamming", 640, 480, 31, 0.5, 40.0)
    for _ in range(120):
        W.pair("ten", 10)
    W.new_row()
    W.pair("ham74", 10, ham=74)
    W.pair("ham75", 10, ham=75, expect=NO_DESCRIPTOR_MATCH)

    def row(n, matched, tie=None):
        """a tile row with n right keypoints 4 px apart; `matched` of them have a left partner (aligned sum 0).  tie =
        (first, last): the left keypoint of column 40 has two right candidates with one descriptor, the true one and a
        decoy 8 px to its left, placed first and last in the row's index order as named."""
        y = W.take_row()                 # (x = 24 + 4 j: the right keypoint of column 0 sits at x = 12, the edge of the domain)
        entries = [("pair", j) if j in matched else ("decoy", j) for j in range(n - (2 if tie else 0))]
        if tie:
            d = W.desc()
            dR = W.flipped(d, 3)
            W.add_left(F(24 + 4 * 40), F(y), d, f"tie{n}:{tie[0]}_first", ACCEPTED if tie[0] == "true" else None)
            xr = 24 + 4 * 40 - D
            place = {"true": F(xr), "decoy": F(xr - 8)}
            entries = [("tie", tie[0])] + entries + [("tie", tie[1])]
        for kind, j in entries:
            if kind == "tie":
                W.add_right(place[j], F(y), dR)
            elif kind == "pair":
                W.pair(f"tierow{n}" if tie else f"row{n}", 0, at=(24 + 4 * j, y))
            else:
                W.add_right(F(24 + 4 * j - D), F(y), W.desc())
    row(1, {0})
    row(63, {62})
    row(64, {63})
    row(65, set(range(65)))          # whichever candidate a truncated loop loses, one of these loses its match
    row(129, {126, 127, 128})
    row(2, set(), ("true", "decoy"))
    row(2, set(), ("decoy", "true"))
    row(65, {1}, ("true", "decoy"))
    row(129, {1}, ("decoy", "true"))
    return W


def world_gates16():
    """maxD = 16: uR on minU and maxU and one float step outside each; zero disparity on a mirror-symmetric tile"""
    W = World("gates16", 320, 240, 41, 0.5, 8.0)
    for i in range(12):
        W.pair("ten", 10)
    for kind in ("on", "below"):
        W.new_row()
        xl, y = X0 + 22 * 3, W.take_row()
        W.make_sum(xl - D, y, 10)
        d = W.desc()
        x = F(xl - 16)
        W.add_right(x if kind == "on" else np.nextafter(x, F(-1e9)), F(y), d)
        W.add_left(F(xl), F(y), d, f"minU:{kind}", ACCEPTED if kind == "on" else NO_DESCRIPTOR_MATCH)
    for kind in ("on", "above"):
        y, x0 = W.take_row(), 100
        W.tile(x0, x0, y, half_r=15, mirror=True)
        d = W.desc()
        W.add_right(F(x0) if kind == "on" else np.nextafter(F(x0), F(1e9)), F(y), d)
        W.add_left(F(x0), F(y), d, f"maxU:{kind}", ACCEPTED_ZERO_DISPARITY if kind == "on" else NO_DESCRIPTOR_MATCH)
    return W


def world_maxd():
    """maxD = 17 with uL in [16, 32): the float steps of uL and of maxD are both 2^-19 and bestuR is an integer, so the
    disparity can sit exactly one step below maxD.  A mirror-symmetric strip centred at x = 8 in the right image (d1 = d3,
    deltaR = 0) under a right keypoint at x = 12, the smallest x of the domain at octave 0: best offset -4, bestuR = 8."""
    W = World("maxd", 320, 240, 51, 0.5, 8.5)
    f25 = F(25)
    for kind, uL, expect in (("below", np.nextafter(f25, F(0)), ACCEPTED), ("on", f25, DISPARITY_OUT),
                             ("above", np.nextafter(f25, F(99)), DISPARITY_OUT)):
        y = W.take_row()
        W.tile(25, 8, y, half_r=6, mirror=True)
        W.make_sum(8, y, 10, symmetric=True)
        d = W.desc()
        W.add_right(F(12), F(y), d)
        W.add_left(uL, F(y), d, f"maxD:{kind}", expect)
    for i in range(4):                     # hold the median at 10
        y = W.take_row()
        W.tile(60, 54, y, half_r=10)
        W.make_sum(54, y, 10)
        d = W.desc()
        W.add_right(F(54), F(y), d)
        W.add_left(F(60), F(y), d, "ten", ACCEPTED)
    return W


def world_gates80(h=300):
    """maxD = 80 on 320 x 300 (the row scan's segments are 2 rows, the last thread's is cut short): octave gate, iniu, endu,
    best offset at the ends of the slide, row bands cut by the first and the last row"""
    W = World("gates80", 320, h, 61, 0.5, 40.0)
    w = W.w
    for i in range(14):
        W.pair("ten", 10)
    W.new_row()
    # right octave against levelL = 0
    W.pair("octR:+1", 10, octave_r=1)
    W.pair("octR:+2", 10, octave_r=2, expect=NO_DESCRIPTOR_MATCH)
    W.new_row()
    # right keypoint beside the true place: 4 px is inside the slide, 5 px is its end
    for dx, expect in ((-5, BEST_AT_END), (-4, ACCEPTED), (4, ACCEPTED), (5, BEST_AT_END)):
        W.pair(f"inc:{-dx:+d}", 10, kp_dx=dx, expect=expect)
        W.new_row()
    # three offsets share the smallest sum (0 at -3, 0 and +3): the first one is the match
    y = W.take_row()
    W.tile_periodic(X0 + 66, X0 + 66 - D, y)
    d = W.desc()
    W.add_right(F(X0 + 66 - D), F(y), d)
    W.add_left(F(X0 + 66), F(y), d, "sadtie", ACCEPTED)
    # a right keypoint with negative x: iniu < 0
    y = W.take_row()
    d = W.desc()
    W.add_right(F(-3), F(y), d)
    W.add_left(F(24), F(y), d, "iniu<0", WINDOW_OUT)
    # endu == cols - 1 is inside, endu == cols is not (level 0: a tile with disparity 5 at the right border)
    for xr, expect in ((w - 12, ACCEPTED), (w - 11, WINDOW_OUT)):
        y = W.take_row()
        W.tile(xr + 5, xr, y, half_r=min(10, w - 1 - xr))
        W.make_sum(xr, y, 10)
        d = W.desc()
        W.add_right(F(xr), F(y), d)
        W.add_left(F(xr + 5), F(y), d, f"endu0:{'cols-1' if expect == ACCEPTED else 'cols'}", expect)
    # the same at level 1 (no pixel-exact outcome for the one that passes: the restatement decides)
    w1, h1 = W.sizes()[1]
    for cu, expect in ((w1 - 12, None), (w1 - 11, WINDOW_OUT)):
        y = W.take_row()
        d = W.desc()
        W.add_right(F(cu) * SCALE[1], F(y), d, octave=1)
        W.add_left(F(w1 - 8) * SCALE[1], F(y), d, f"endu1:{'cols-1' if expect is None else 'cols'}", expect, octave=1)
    # levelL at the top level: right octaves 5 (gated), 6 and 7.  Both eyes hold the same pixels in a block around the place,
    # so the two pyramids agree there at every level and the aligned sum at level 7 is 0; uL sits 0.45 level-7 px right of
    # the window's centre, which keeps the disparity positive for every deltaR below 0.45.
    top = NLEVELS - 1
    W.right[215:286, 70:216] = W.left[215:286, 70:216]
    for o, expect in ((top - 2, NO_DESCRIPTOR_MATCH), (top - 1, ACCEPTED), (top, ACCEPTED)):
        d = W.desc()
        W.add_right(F(40) * SCALE[top], F(250), d, octave=o)
        W.add_left(F(40.45) * SCALE[top], F(250), d, f"octL7:{o - top:+d}", expect, octave=top)
    # bands cut by the borders: only y is used.  A right keypoint of octave 1 at y = h - 3 reaches down to row h - 6, where the
    # last left keypoint that is in the domain sits; octave 0 at y = 1 is cut by row 0 and no left keypoint looks at it.
    W.add_right(F(50), F(1.0), W.desc())
    W.add_right(F(50), F(0.0), W.desc(), octave=2)
    xl, y = X0 + 22 * 4, h - 6
    W.pair("band_bottom", 10, at=(xl, y), octave_r=1, yr=h - 3)
    W.add_right(F(200), F(h - 1), W.desc())
    return W


def world_nright1():
    W = World("nright1", 320, 240, 71, 0.5, 40.0)
    W.pair("only", 10)
    xl, y = W.take_tile()
    W.add_left(F(xl), F(y), W.desc(), "other", NO_DESCRIPTOR_MATCH)
    W.add_left(F(100), F(W.take_row()), W.desc(), "empty_row", NO_CANDIDATES)
    return W


def world_levels():
    """No planted keypoint: the extractors' own keypoints supply the levels that cannot be planted pixel-exactly.  On the
    shifted noise alone only levels 0 and 1 get a match (a 12 px shift of white noise leaves nothing for the descriptors of the
    coarser levels to agree on), so below row 380 both eyes hold the same pixels: there the two pyramids agree at every level."""
    W = World("levels", 640, 480, 81, 0.5, 40.0, nfeatures=1000)
    W.right[380:, :] = W.left[380:, :]
    return W


MEDIAN_WORLDS = {
    # name: (sums, indices made by one +s edit, culled sums)
    "odd":      ((5, 10, 10, 20, 21), (0, 3, 4), (21,)),
    "even":     ((5, 10, 10, 20, 21, 22), (3,), ()),           # element nv/2 is 20: thDist = 42
    "one":      ((10,), (), ()),
    "two":      ((3, 7), (1,), ()),                             # element 1 is 7: thDist = 14.7
    "zeros":    ((0, 0, 0, 4), (3,), (0, 0, 0, 4)),             # median 0: thDist = 0, `<` keeps nothing
    "tied":     ((5, 10, 10, 10, 21, 25), (4,), (21, 25)),      # the median value holds ranks 1 .. 3
}


def build_worlds():
    """name -> World, every call builds the same bytes"""
    out = {}
    for i, (name, (sums, singles, culled)) in enumerate(MEDIAN_WORLDS.items()):
        out["median_" + name] = _sums_world("median_" + name, sums, 100 + i, singles, culled)
    for f in (world_pixels, world_nomatch, world_hamming, world_gates16, world_maxd, world_gates80, world_nright1, world_levels):
        W = f()
        out[W.name] = W
    return out


N_LEFT_PREFIXES = (1, 3, 4, 5, 255, 256, 257)     # of the `pixels` world: 4 left keypoints per workgroup, the cull strides by 256


# ---------------------------------------------------------------------------------------------------------------------
# Shared by the CPU and the GPU tests

def oracle_side(oracle, W):
    """both oracle extractors on the world's pair -> (eL, eR, planes_l, planes_r, natural keypoints of both eyes)"""
    eL, eR = oracle.Extractor(nfeatures=W.nfeatures), oracle.Extractor(nfeatures=W.nfeatures)
    nat = eL.extract(W.left) + eR.extract(W.right)
    assert np.array_equal(eL.scale_factors, SCALE) and np.array_equal(eL.inv_scale_factors, INV_SCALE)
    assert [eL.level_size(l)[:2] for l in range(NLEVELS)] == W.sizes()
    return eL, eR, [eL.level_plane(l) for l in range(NLEVELS)], [eR.level_plane(l) for l in range(NLEVELS)], nat


def check_expectations(W, trace):
    """every planted keypoint that names the reason it was planted for ends with it"""
    for i, want in enumerate(W.expect):
        if want is not None:
            assert trace["reason"][i] == want, (W.name, W.tags[i], REASONS[trace["reason"][i]], REASONS[want])
