"""Shared by tests/test_dbow2_ref_cpu.py, tests/test_dbow2_ref_gpu.py and tests/golden/make_golden.py: the cases that pin the
vocabulary path against the reference's own DBoW2 (the driver oracle/_ref/dbow2_ref, built by `make -C oracle dbow2_ref`),
the call that runs one case through the driver, the fixture layout of tests/golden/dbow2_ref_*.npz, and the comparisons.

A *case* is one driver invocation: a vocabulary file (its exact bytes), the loader that reads it, an optional
setScoringType / setWeightingType override, descriptor sets with their levelsup, and pairs of sets to score.  Everything
is compared bit for bit (doubles as raw bytes)."""
import os
import subprocess

import numpy as np

import bundle_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "dbow2_ref")
REF_DIR = os.environ.get("AOS2_REFERENCE_DIR", "/root/reference")
COUNTS = (0, 1, 15, 16, 17, 255, 256, 257, 511, 513, 600)   # 16 features per workgroup of the descent; 256-thread chunks
#                                                             and the power-of-two padding of the assembly sort
HEADER_REFUSED = {"k21": "21 3 0 0", "L0": "10 0 0 0", "L11": "10 11 0 0", "scoring6": "10 3 6 0", "weighting4": "10 3 0 4"}


def live_binary():
    """Path of the driver, or None when neither it nor the reference's sources are there (the only reason to skip)."""
    if os.path.exists(REF_BIN):
        return REF_BIN
    if os.path.isdir(REF_DIR):
        raise AssertionError(f"{REF_BIN} is missing although {REF_DIR} exists: __graft_entry__.build() makes it")
    return None


SKIP_REASON = f"neither the driver {REF_BIN} nor the reference's sources {REF_DIR} are present"


# ---------------------------------------------------------------------------------------------------------- trees
def _synth():
    import __graft_entry__ as graft
    return graft.load_package().synth


def make_tree(seed, k, L, ragged=False, tie=False, n_stopped=3, inner_last=False, double_weights=False):
    """synth_vocabulary plus: the first `n_stopped` words stopped (weight 0) whatever the seed gave; tie=True gives the
    first ten children of the root one descriptor; inner_last=True appends a childless record whose leaf flag is 0
    (what a text file whose last record is an inner node looks like); double_weights=True gives weights no float holds
    (synth_vocabulary's are float-exact), so that the binary format's double -> float -> double shows."""
    voc = _synth().synth_vocabulary(seed, k, L, ragged=ragged)
    voc = {n: (np.array(v) if isinstance(v, np.ndarray) else v) for n, v in voc.items()}
    leaves = np.flatnonzero(voc["is_leaf"])
    voc["weight"][leaves[:n_stopped]] = 0.0
    if tie:
        voc["desc"][1:10] = voc["desc"][0]
    if double_weights:
        voc["weight"] = voc["weight"] * np.random.default_rng(seed + 2000).uniform(1.0, 1.001, len(voc["weight"]))
    if inner_last:
        rng = np.random.default_rng(seed + 1000)
        voc["parent"] = np.append(voc["parent"], np.int32(0)).astype(np.int32)
        voc["desc"] = np.concatenate([voc["desc"], rng.integers(0, 256, size=(1, 32), dtype=np.uint8)])
        voc["weight"] = np.append(voc["weight"], 0.0)
        voc["is_leaf"] = np.append(voc["is_leaf"], np.uint8(0)).astype(np.uint8)
    return voc


def text_bytes(voc, scoring=0, weighting=0, final_newline=False, header=None):
    lines = [header if header is not None else f'{voc["k"]} {voc["L"]} {scoring} {weighting}']
    for i in range(len(voc["parent"])):
        lines.append(f'{voc["parent"][i]} {int(voc["is_leaf"][i])} ' + " ".join(str(int(x)) for x in voc["desc"][i]) +
                     f' {float(voc["weight"][i])!r}')
    return ("\n".join(lines) + ("\n" if final_newline else "")).encode()


_REC = np.dtype([("parent", "<i4"), ("desc", "u1", 32), ("weight", "<f4"), ("leaf", "u1")])   # 41 bytes, packed


def binary_bytes(voc, scoring=0, weighting=0):
    """The layout of saveToBinaryFile (TemplatedVocabulary.h:1514-1534), written independently of either writer under test:
    the leaf byte is isLeaf(), i.e. "has no children", not the text file's flag."""
    n = len(voc["parent"])
    rec = np.zeros(n, _REC)
    rec["parent"], rec["desc"], rec["weight"] = voc["parent"], voc["desc"], voc["weight"].astype(np.float32)
    rec["leaf"] = ~np.isin(np.arange(1, n + 1), voc["parent"])
    hdr = np.array([n + 1, 41, voc["k"], voc["L"], scoring, weighting], "<i4")
    return hdr.tobytes() + rec.tobytes()


def depth_of_nodes(parent):
    """depth of node 1..n (root = 0) from `parent` of nodes 1..n"""
    d = np.zeros(len(parent) + 1, np.int64)
    for i, p in enumerate(parent):
        d[i + 1] = d[p] + 1
    return d


# ---------------------------------------------------------------------------------------------------------- sets
def descriptor_sets(voc, seed, counts=COUNTS, n_all_lu=257, n_repeat=300):
    """[(desc, levelsup)]: one set per count with levelsup cycling through 0, 1, 2, L - 1, L, L + 3, all six on one more set,
    one set with 40 copies of one descriptor, one that lands only on stopped words."""
    S = _synth()
    rng = np.random.default_rng(seed)
    L = voc["L"]
    lus = (0, 1, 2, L - 1, L, L + 3)
    sets = []
    for i, n in enumerate(counts):
        sets.append((S.vocab_descriptors(rng, voc, n), lus[i % 6]))
    d = S.vocab_descriptors(rng, voc, n_all_lu)
    sets += [(d, lu) for lu in lus]
    d = S.vocab_descriptors(rng, voc, n_repeat)
    d[20:60] = d[20]                                        # w + w + ... forty times, in double
    sets.append((d, 2))
    stopped = np.flatnonzero((voc["is_leaf"] > 0) & (voc["weight"] == 0))
    sets.append((voc["desc"][stopped[np.arange(33) % len(stopped)]].copy(), 1))
    return sets


def score_sets(voc, seed, na=300, nb=211, shared=90):
    """([(desc, levelsup)] * 5, pairs): identical, partially overlapping, disjoint and empty BowVectors, distinct n."""
    S = _synth()
    rng = np.random.default_rng(seed)
    a = S.vocab_descriptors(rng, voc, na)
    b = S.vocab_descriptors(rng, voc, nb)
    b[:shared] = a[:shared]
    # disjoint: the exact descriptors of words below the first and below the last child of the root
    first_child = np.flatnonzero(voc["parent"] == 0)
    top = np.arange(1, len(voc["parent"]) + 1)
    for _ in range(voc["L"]):
        par = voc["parent"][top - 1]
        top = np.where(par == 0, top, par)
    words = (voc["is_leaf"] > 0) & (voc["weight"] > 0)
    lo = np.flatnonzero(words & (top == first_child[0] + 1))[:57]
    hi = np.flatnonzero(words & (top == first_child[-1] + 1))[:23]
    sets = [(a, 4), (b, 4), (voc["desc"][lo].copy(), 4), (voc["desc"][hi].copy(), 4), (np.zeros((0, 32), np.uint8), 4)]
    pairs = np.array([[0, 0], [0, 1], [1, 0], [2, 3], [0, 4], [4, 4], [2, 0]], np.int32)
    return sets, pairs


def make_case(name, voc, file_bytes, binary, sets=(), pairs=None, set_scoring=-1, set_weighting=-1, save=False, pre=None):
    c = dict(name=name, voc=voc, file=np.frombuffer(file_bytes, np.uint8).copy(), binary=int(binary), sets=list(sets),
             pairs=pairs, set_scoring=set_scoring, set_weighting=set_weighting, save=int(save), pre=pre)
    return c


# ---------------------------------------------------------------------------------------------------------- driver
def run_ref(case, tmpdir, binary_path=None):
    """Run one case through the reference driver -> dict of its recorded outputs."""
    tmpdir = str(tmpdir)
    fpath = os.path.join(tmpdir, case["name"] + (".bin" if case["binary"] else ".txt"))
    with open(fpath, "wb") as f:
        f.write(case["file"].tobytes())
    arrs = dict(voc_path=np.frombuffer(fpath.encode(), np.uint8), binary=np.array([case["binary"]], np.int32),
                set_scoring=np.array([case["set_scoring"]], np.int32), set_weighting=np.array([case["set_weighting"]], np.int32),
                save=np.array([case["save"]], np.int32))
    if case["pre"] is not None:
        pre_bytes, pre_binary = case["pre"]
        ppath = os.path.join(tmpdir, case["name"] + ".pre")
        with open(ppath, "wb") as f:
            f.write(bytes(pre_bytes))
        arrs.update(pre_path=np.frombuffer(ppath.encode(), np.uint8), pre_binary=np.array([int(pre_binary)], np.int32))
    if case["sets"]:
        arrs["desc"] = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d, _ in case["sets"]])
        arrs["set_off"] = np.concatenate([[0], np.cumsum([len(d) for d, _ in case["sets"]])]).astype(np.int32)
        arrs["levelsup"] = np.array([lu for _, lu in case["sets"]], np.int32)
    if case["pairs"] is not None:
        arrs["pairs"] = np.asarray(case["pairs"], np.int32)
    ipath, opath = os.path.join(tmpdir, case["name"] + ".in"), os.path.join(tmpdir, case["name"] + ".out")
    bundle_io.save(ipath, arrs)
    r = subprocess.run([binary_path or REF_BIN, ipath, opath], capture_output=True, text=True)
    assert r.returncode == 0, f"dbow2_ref failed ({r.returncode}): {r.stderr}"
    return bundle_io.load(opath)


# ---------------------------------------------------------------------------------------------------------- fixtures
_VOC_KEYS = ("parent", "desc", "weight", "is_leaf")
FIXTURES = ("dbow2_ref_trees_a.npz", "dbow2_ref_trees_b.npz", "dbow2_ref_trees_c.npz", "dbow2_ref_variants.npz",
            "dbow2_ref_loader.npz")


def save_fixture(path, cases_and_outputs):
    """tests/golden/dbow2_ref_*.npz: data only -- per case the vocabulary arrays, the exact bytes of the vocabulary file,
    the descriptor sets and what the driver recorded.  Arrays are stored once per content (`blob_<sha1>`); `index` maps
    "<case>/<key>" to its blob, so the cases of one file share their tree and their descriptors."""
    import hashlib
    blobs, index = {}, []

    def put(case, key, a):
        a = np.ascontiguousarray(a)
        h = "blob_" + hashlib.sha1(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()[:16]
        blobs[h] = a
        index.append(f"{case}/{key}={h}")

    for c, out in cases_and_outputs:
        nm = c["name"]
        for k in _VOC_KEYS:
            put(nm, "voc." + k, c["voc"][k])
        put(nm, "meta", np.array([c["voc"]["k"], c["voc"]["L"], c["binary"], c["set_scoring"], c["set_weighting"], c["save"],
                                  len(c["sets"])], np.int32))
        put(nm, "file", c["file"])
        if c["pre"] is not None:
            put(nm, "pre", np.frombuffer(bytes(c["pre"][0]), np.uint8))
            put(nm, "pre_binary", np.array([int(c["pre"][1])], np.int32))
        for s, (d, lu) in enumerate(c["sets"]):
            put(nm, f"set{s}", np.asarray(d, np.uint8).reshape(-1, 32))
            put(nm, f"lu{s}", np.array([lu], np.int32))
        if c["pairs"] is not None:
            put(nm, "pairs", np.asarray(c["pairs"], np.int32))
        for k, v in out.items():
            put(nm, "out." + k, v)
    np.savez_compressed(path, names=np.array([c["name"] for c, _ in cases_and_outputs]), index=np.array(index), **blobs)


_loaded = {}


def load_fixture(name):
    """-> [(case, recorded outputs)], read once per process and shared (nothing modifies them)"""
    if name in _loaded:
        return _loaded[name]
    z = np.load(os.path.join(GOLD, name))
    per = {}
    for e in z["index"]:
        key, h = str(e).split("=")
        case, key = key.split("/", 1)
        per.setdefault(case, {})[key] = z[h]
    res = []
    for nm in z["names"]:
        nm = str(nm)
        a = per[nm]
        m = a["meta"]
        voc = {k: a["voc." + k] for k in _VOC_KEYS}
        voc.update(k=int(m[0]), L=int(m[1]), scoring=0, weighting=0)
        sets = [(a[f"set{s}"], int(a[f"lu{s}"][0])) for s in range(int(m[6]))]
        pre = (a["pre"].tobytes(), int(a["pre_binary"][0])) if "pre" in a else None
        c = dict(name=nm, voc=voc, file=a["file"], binary=int(m[2]), set_scoring=int(m[3]), set_weighting=int(m[4]),
                 save=int(m[5]), sets=sets, pairs=a.get("pairs"), pre=pre)
        res.append((c, {k[4:]: v for k, v in a.items() if k.startswith("out.")}))
    _loaded[name] = res
    return res


# ---------------------------------------------------------------------------------------------------------- case lists
def near_leaf_sets(voc, seed, counts=(0, 1, 17, 65), levelsup=1):
    """descriptors a few bits away from words of the vocabulary (no unrelated ones: they stay clear of a zero descriptor)"""
    S = _synth()
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(voc["is_leaf"])
    return [(S.flip_bits(rng, voc["desc"][rng.choice(leaves, n)], 0.03), levelsup) for n in counts]


def transform_cases(small):
    """Trees x descriptor counts x levelsup.  small=True is the subset the fixtures record."""
    if small:
        kw = dict(counts=(0, 1, 16, 17, 65), n_all_lu=33, n_repeat=80)
        trees = [("ragged_k6_L3", make_tree(3, 6, 3, ragged=True), 0), ("k20_L2", make_tree(4, 20, 2), 0),
                 ("tie_k10_L2", make_tree(11, 10, 2, tie=True), 0), ("k65_L1", make_tree(6, 65, 1), 1)]
    else:
        kw = dict(counts=COUNTS, n_all_lu=257, n_repeat=300)
        trees = [("k10_L3", make_tree(1, 10, 3), 0), ("k4_L6", make_tree(2, 4, 6), 0), ("k18_L3", make_tree(7, 18, 3), 0),
                 ("k2_L10", make_tree(8, 2, 10), 0), ("k20_L2", make_tree(4, 20, 2), 0),
                 ("ragged_k10_L4", make_tree(9, 10, 4, ragged=True), 0), ("tie_k10_L2", make_tree(11, 10, 2, tie=True), 0),
                 ("k33_L2", make_tree(12, 33, 2), 1), ("k65_L1", make_tree(6, 65, 1), 1)]
    cases = []
    for i, (name, voc, binary) in enumerate(trees):
        data = binary_bytes(voc) if binary else text_bytes(voc)
        if small and i == 0:
            kw = dict(kw, counts=(0, 1, 17, 257))
        cases.append(make_case(name, voc, data, binary, descriptor_sets(voc, 40 + i, **kw)))
    return cases


def variant_cases(small):
    """All 6 scorings x 4 weightings, each once through the file header ("h") and once through setScoringType /
    setWeightingType on a file that says 0 0 ("s")."""
    voc = make_tree(5, 5, 2) if small else make_tree(1, 10, 3)
    rng = np.random.default_rng(77)
    d = _synth().vocab_descriptors(rng, voc, 120 if small else 300)
    d[20:60] = d[20]
    sets = [(d, 2), (d[:17].copy(), 2)]     # one levelsup: the two sets also serve as one transform_device batch
    body = text_bytes(voc).split(b"\n", 1)[1]
    cases = []
    for sc in range(6):
        for wt in range(4):
            hdr = f'{voc["k"]} {voc["L"]} {sc} {wt}\n'.encode()
            cases.append(make_case(f"h_s{sc}_w{wt}", voc, hdr + body, 0, sets))
            cases.append(make_case(f"s_s{sc}_w{wt}", voc, text_bytes(voc), 0, sets, set_scoring=sc, set_weighting=wt))
    return cases


def loader_cases():
    """Both loaders and the writer on a tree whose last record is a leaf and on one whose last record is an inner node (a
    childless record with leaf flag 0, a child of the root): text without and with the final newline, and binary."""
    cases = []
    for tag, inner in (("leaflast", False), ("innerlast", True)):
        voc = make_tree(5, 4, 2, inner_last=inner, double_weights=True)
        assert (voc["weight"].astype(np.float32).astype(np.float64) != voc["weight"]).sum() > 10
        sets = near_leaf_sets(voc, 5)
        zero = [(np.zeros((9, 32), np.uint8), 1)]    # the phantom's descriptor: only where its parent is defined (the root)
        cases.append(make_case(f"{tag}_text", voc, text_bytes(voc, 2, 1), 0, sets + zero, save=True))
        cases.append(make_case(f"{tag}_text_nl", voc, text_bytes(voc, 2, 1, final_newline=True), 0, sets + (zero if inner else []),
                               save=True))
        cases.append(make_case(f"{tag}_binary", voc, binary_bytes(voc, 2, 1), 1, sets + zero, save=True))
    return cases


def header_cases():
    """Headers loadFromTextFile refuses, on a fresh vocabulary and on one that holds a tree with scoring 2, weighting 1."""
    voc = make_tree(5, 4, 2)
    good = text_bytes(voc, 2, 1)
    sets = near_leaf_sets(voc, 6, counts=(5,))
    cases = []
    for tag, hdr in HEADER_REFUSED.items():
        cases.append(make_case(f"refused_{tag}_fresh", voc, text_bytes(voc, header=hdr), 0, sets))
        cases.append(make_case(f"refused_{tag}_loaded", voc, text_bytes(voc, header=hdr), 0, sets, pre=(good, 0)))
    return cases


def score_case(small):
    voc = make_tree(13, 6, 3) if small else make_tree(1, 10, 3)
    sets, pairs = score_sets(voc, 21, *((60, 41, 15) if small else (300, 211, 90)))
    return make_case("score_l1", voc, text_bytes(voc), 0, sets, pairs=pairs)


def fixture_cases():
    """{fixture file: [case]}"""
    t = transform_cases(True)
    return {"dbow2_ref_trees_a.npz": [t[0], t[3]], "dbow2_ref_trees_b.npz": [t[1]], "dbow2_ref_trees_c.npz": [t[2], score_case(True)],
            "dbow2_ref_variants.npz": variant_cases(True),
            "dbow2_ref_loader.npz": loader_cases() + header_cases()}


# ---------------------------------------------------------------------------------------------------------- comparisons
def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def check_tree(info, nodes, out, what=""):
    """info: dict(k, L, scoring, weighting, nodes, words); nodes: dict(parent, is_leaf, word_id, weight, desc) over all
    m_nodes (root included) of the implementation under test; out: the driver's record."""
    for key, okey in (("k", "k"), ("L", "L"), ("scoring", "scoring"), ("weighting", "weighting"), ("nodes", "n_nodes"),
                      ("words", "size")):
        assert info[key] == int(out[okey][0]), f"{what}: {key} {info[key]} != reference {int(out[okey][0])}"
    same(nodes["parent"].astype(np.int32), out["node_parent"], what + ": parent of every node")
    same(nodes["is_leaf"].astype(np.int32), out["node_leaf"], what + ": isLeaf() of every node")
    same(nodes["word_id"].astype(np.int32), out["node_word"], what + ": word id of every node")
    same(nodes["weight"], out["node_weight"], what + ": weight of every node (raw bits)")
    same(nodes["desc"].reshape(-1, 32), out["node_desc"], what + ": descriptor of every node")


def defined_nid_mask(out, s, L, levelsup):
    """Features of set s whose FeatureVector node the reference defines.  transform(feature, id, weight, &nid, levelsup)
    assigns *nid only when the descent reaches level L - levelsup (or that level is <= 0: the root).  A feature whose
    leaf lies above that level leaves `NodeId nid;` of the caller unassigned: the value is indeterminate there (whatever
    the stack held), not a convention, so nothing is compared for it."""
    word_of, weight_of = out[f"s{s}.word_of"], out[f"s{s}.weight_of"]
    # the driver starts *nid as -1, which survives exactly where the reference does not assign it
    mask = out[f"s{s}.node_of"] != -1
    if int(out["size"][0]) == 0:   # empty vocabulary: transform clears both outputs and descends nowhere
        return np.zeros(len(word_of), bool)
    nid_level = L - levelsup
    if nid_level <= 0:
        assert mask.all()
        return mask
    # cross-check by depth for the features that enter the FeatureVector (weight > 0: their leaf is a word, and a word
    # id names one node; childless non-words all report word id 0 and weight 0)
    depth = depth_of_nodes(out["node_parent"][1:])
    leaf_of_word = {}
    for nid in np.flatnonzero((out["node_leaf"] != 0) & (out["node_weight"] > 0)):
        leaf_of_word.setdefault(int(out["node_word"][nid]), int(nid))
    for i in np.flatnonzero(weight_of > 0):
        assert (depth[leaf_of_word[int(word_of[i])]] >= nid_level) == mask[i], "mask by depth != where the reference assigned nid"
    return mask


def check_transform(got, out, s, L, levelsup, what=""):
    """got: dict(bow_word, bow_value, fv_node, fv_off, fv_idx, word_of, node_of) of the implementation under test."""
    p = f"s{s}."
    w = f"{what} set {s} (n={len(out[p + 'word_of'])}, levelsup={levelsup})"
    same(got["bow_word"].astype(np.int32), out[p + "bow_word"], w + ": BowVector words")
    same(got["bow_value"], out[p + "bow_value"], w + ": BowVector values (raw bits)")
    same(got["word_of"].astype(np.int32), out[p + "word_of"], w + ": word of every feature")
    mask = defined_nid_mask(out, s, L, levelsup)
    stopped = out[p + "weight_of"] <= 0
    n = len(mask)
    same(got["node_of"].astype(np.int32)[mask], out[p + "node_of"][mask], w + ": node of every feature")
    # FeatureVector: the same features are kept; their nodes agree wherever the reference defines them
    assert got["fv_off"][0] == 0 and len(got["fv_off"]) == len(got["fv_node"]) + 1 and got["fv_off"][-1] == len(got["fv_idx"]), w
    assert (np.diff(got["fv_node"]) > 0).all(), w + ": FeatureVector nodes ascend"
    node_g, node_r = np.full(n, -2, np.int64), np.full(n, -2, np.int64)
    for j in range(len(got["fv_node"])):
        seg = got["fv_idx"][got["fv_off"][j]: got["fv_off"][j + 1]]
        assert len(seg) > 0 and (np.diff(seg) > 0).all(), w + ": features of a node ascend"
        node_g[seg] = got["fv_node"][j]
    for j in range(len(out[p + "fv_node"])):
        node_r[out[p + "fv_idx"][out[p + "fv_off"][j]: out[p + "fv_off"][j + 1]]] = out[p + "fv_node"][j]
    same(node_g >= -1, node_r >= -1, w + ": features kept in the FeatureVector")
    same(node_g >= -1, ~stopped, w + ": exactly the non-stopped features are kept")
    same(node_g[mask], node_r[mask], w + ": FeatureVector node of every feature")
    if mask.all():
        same(got["fv_node"], out[p + "fv_node"], w + ": fv_node")
        same(got["fv_off"], out[p + "fv_off"], w + ": fv_off")
        same(got["fv_idx"], out[p + "fv_idx"], w + ": fv_idx")


# ---------------------------------------------------------------------------------------------------------- one case, one implementation
class Impl:
    """The implementation under test behind one face: `lib` is the package (pkg.Vocabulary, the HIP library) or the
    oracle module (oracle.Vocabulary, oracle/dbow_oracle.c)."""

    def __init__(self, lib, is_oracle):
        self.lib, self.is_oracle = lib, is_oracle

    def new(self):
        return self.lib.Vocabulary()

    def load(self, v, path, binary):
        if self.is_oracle:
            return v.load_binary(path) if binary else v.load_text(path)
        return v.loadFromBinaryFile(path) if binary else v.loadFromTextFile(path)

    def save(self, v, path):
        if self.is_oracle:
            assert v.save_binary(path)
        else:
            v.saveToBinaryFile(path)

    def score(self, v, a, b):
        return self.lib.vocab_score_l1(a, b) if self.is_oracle else v.score(a, b)

    def transform(self, v, d, levelsup):
        r = v.transform(d, levelsup)
        if r is None:   # the oracle's answer for an empty vocabulary: both outputs cleared
            n = len(d)
            r = dict(bow_word=np.zeros(0, np.uint32), bow_value=np.zeros(0), fv_node=np.zeros(0, np.int32),
                     fv_off=np.zeros(1, np.int32), fv_idx=np.zeros(0, np.int32), word_of=np.zeros(n, np.uint32),
                     node_of=np.zeros(n, np.uint32))
        return r


def phantom_parent_defined(case):
    """Text files with a final newline give one more node.  The reference reads its parent from an `int pid`
    that no `>>` assigned: indeterminate.  The build keeps the previous record's value in it, so the node lands below the
    root -- our convention -- exactly when the last record is a child of the root; only there is the parent compared."""
    if case["binary"] or not case["file"].tobytes().endswith(b"\n"):
        return None
    return int(case["voc"]["parent"][-1]) == 0


def ref_bow(out, s):
    return dict(bow_word=out[f"s{s}.bow_word"].view(np.uint32), bow_value=out[f"s{s}.bow_value"])


def check_case(impl, case, out, tmpdir, host_only=False):
    """Load the case's file into the implementation under test and compare everything the driver recorded.  host_only:
    no transform (it needs the device); loaders, tree, writer, and score() on the reference's BowVectors."""
    what = case["name"]
    tmpdir = str(tmpdir)
    v = impl.new()
    path = os.path.join(tmpdir, what + ".impl" + (".bin" if case["binary"] else ".txt"))
    with open(path, "wb") as f:
        f.write(case["file"].tobytes())
    if case["pre"] is not None:
        ppath = os.path.join(tmpdir, what + ".impl.pre")
        with open(ppath, "wb") as f:
            f.write(bytes(case["pre"][0]))
        assert impl.load(v, ppath, case["pre"][1])
    ok = impl.load(v, path, case["binary"])
    assert bool(ok) == bool(out["loaded"][0]), f"{what}: load returned {ok}, the reference {bool(out['loaded'][0])}"
    if case["set_scoring"] >= 0 or case["set_weighting"] >= 0:
        # no setter in our API: the same tree, built with the scoring / weighting the reference was set to
        voc = case["voc"]
        v = impl.new()
        v.set_nodes(voc["k"], voc["L"], case["set_scoring"], case["set_weighting"], voc["parent"], voc["desc"], voc["weight"],
                    voc["is_leaf"])
    nodes = v.nodes()
    ph = phantom_parent_defined(case)
    ref = dict(out)
    if ph is not None:
        # what the reference defines for the node after the final newline: it exists, has no children and weight 0;
        # its descriptor is zero under the stand-in Mat (a real cv::Mat::create leaves it unset)
        assert int(out["n_nodes"][0]) == len(case["voc"]["parent"]) + 2 and out["node_leaf"][-1] == 1, what
        assert out["node_weight"][-1] == 0 and not out["node_desc"][-1].any(), what
        assert nodes["parent"][-1] == 0, what + ": our phantom node hangs below the root"
        if not ph:
            ref["node_parent"] = out["node_parent"].copy()
            ref["node_parent"][-1] = 0
    check_tree(v.info(), nodes, ref, what)
    got = []
    for s, (d, lu) in enumerate(case["sets"]):
        if host_only:
            got.append(ref_bow(out, s))
            continue
        got.append(impl.transform(v, d, lu))
        check_transform(got[-1], out, s, int(out["L"][0]), lu, what)
    if case["pairs"] is not None:
        for p, (a, b) in enumerate(case["pairs"]):
            same(np.float64(impl.score(v, got[a], got[b])), out["score"][p], f"{what}: score of sets {a}, {b} (raw bits)")
    if case["save"]:
        spath = os.path.join(tmpdir, what + ".impl.saved")
        impl.save(v, spath)
        with open(spath, "rb") as f:
            mine = np.frombuffer(f.read(), np.uint8).copy()
        theirs = out["saved"].copy()
        if ph is False:   # the phantom's parent field of the last record
            theirs[-41:-37] = 0
        same(mine, theirs, what + ": bytes of saveToBinaryFile")
    return v, got
