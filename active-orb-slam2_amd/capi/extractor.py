"""ORBextractor, ORBVocabulary and Frame::ComputeStereoMatches (include/aos2.h: aos2_extractor_*, aos2_vocabulary_*,
aos2_compute_stereo_matches*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import AOS2_OK, KP_DTYPE
from ._core import _Handle, _check, _p, host_empty


class Extractor(_Handle):
    """Mirror of ORBextractor (include/ORBextractor.h:45-111): ctor args, operator(), getters."""

    KIND = "extractor"

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, device=0):
        self._create(nfeatures, scale_factor, nlevels, ini_th, min_th, device)
        self.nlevels = nlevels
        self.nfeatures = nfeatures

    def _arr(self, name, n, dt):
        ptr = getattr(self.L, "aos2_extractor_" + name)(self.h)
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy()

    # GetLevels / GetScaleFactor(s) / ... (include/ORBextractor.h:58-83)
    def GetLevels(self):
        return self.L.aos2_extractor_levels(self.h)

    def GetScaleFactor(self):
        return self.L.aos2_extractor_scale_factor(self.h)

    def GetScaleFactors(self):
        return self._arr("scale_factors", self.nlevels, np.float32)

    def GetInverseScaleFactors(self):
        return self._arr("inv_scale_factors", self.nlevels, np.float32)

    def GetScaleSigmaSquares(self):
        return self._arr("sigma2", self.nlevels, np.float32)

    def GetInverseScaleSigmaSquares(self):
        return self._arr("inv_sigma2", self.nlevels, np.float32)

    @property
    def features_per_level(self):
        return self._arr("features_per_level", self.nlevels, np.int32)

    @property
    def umax(self):
        return self._arr("umax", 16, np.int32)

    @property
    def max_keypoints(self):
        return self.L.aos2_extractor_max_keypoints(self.h)

    def max_keypoints_for(self, w, h):
        """capacity that always suffices for w x h images (wide images can exceed nfeatures + 3 per level)"""
        return self.L.aos2_extractor_max_keypoints_for(self.h, int(w), int(h))

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors): returns (keypoints[KP_DTYPE], desc[n,32])."""
        if image is None or image.size == 0:
            n = C.c_int(-1)
            _check(self.L.aos2_extractor_extract(self.h, None, 0, 0, 0, None, None, 0, C.byref(n)))
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        if image.dtype != np.uint8 or image.ndim != 2:
            raise AssertionError("image.type() == CV_8UC1")  # src/ORBextractor.cc:1050
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        h, w = image.shape
        cap = self.max_keypoints_for(w, h)
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        _check(self.L.aos2_extractor_extract(self.h, _p(image), w, h, image.strides[0], _p(kps), _p(desc), cap, C.byref(n)))
        return kps[: n.value].copy(), desc[: n.value].copy()

    def extract_batch(self, images):
        """host images [B, h, w] (any host memory; host_empty() arrays are uploaded by DMA) -> [(kps, desc)] * B"""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        B, h, w = images.shape
        cap = self.max_keypoints_for(w, h)
        if getattr(self, "_out_key", None) != (B, cap):   # page-locked result buffers, reused between calls
            self._out_key, self._out = None, None
            self._out = (host_empty((B, cap), KP_DTYPE), host_empty((B, cap, 32), np.uint8))
            self._out_key = (B, cap)
        kps, desc = self._out
        n = np.zeros(B, np.int32)
        _check(self.L.aos2_extractor_extract_batch(self.h, _p(images), B, w, h, w, w * h, _p(kps), _p(desc), cap, _p(n)))
        return [(kps[b, : n[b]].copy(), desc[b, : n[b]].copy()) for b in range(B)]

    def extract_batch_device(self, d_imgs, batch, w, h, stride, image_stride, d_kps, d_desc, cap, d_nout):
        """raw device pointers (ints)"""
        _check(self.L.aos2_extractor_extract_batch_device(self.h, C.c_void_p(d_imgs), batch, w, h, stride, image_stride,
                                                          C.c_void_p(d_kps), C.c_void_p(d_desc), cap, C.c_void_p(d_nout)))

    def extract_batch_device_async(self, d_imgs, batch, w, h, stride, image_stride, d_kps, d_desc, cap, d_nout):
        """enqueue only (raw device pointers); results and errors are complete after wait()"""
        _check(self.L.aos2_extractor_extract_batch_device_async(self.h, C.c_void_p(d_imgs), batch, w, h, stride, image_stride,
                                                                C.c_void_p(d_kps), C.c_void_p(d_desc), cap, C.c_void_p(d_nout)))

    def pack_slots(self, batch, d_kps, d_desc, d_n, cap, d_slots, slot_bytes, stream=None):
        """aos2_extractor_pack_slots: device outputs -> fixed-size per-frame slots (sharding.slot_bytes layout)"""
        _check(self.L.aos2_extractor_pack_slots(self.h, batch, d_kps, d_desc, d_n, cap, d_slots, slot_bytes, stream))

    def stream_wait(self, stream):
        _check(self.L.aos2_extractor_stream_wait(self.h, stream))

    def wait_for_stream(self, stream):
        """the batches enqueued from now on run behind what `stream` holds so far (device-side)"""
        _check(self.L.aos2_extractor_wait_for_stream(self.h, stream))

    def wait(self):
        """complete every batch enqueued with extract_batch_device_async"""
        _check(self.L.aos2_extractor_wait(self.h))

    def pyramid_level(self, level, image=0, border=0):
        """mvImagePyramid[level] (include/ORBextractor.h:85)"""
        w, h = C.c_int(), C.c_int()
        _check(self.L.aos2_extractor_pyramid_level_size(self.h, level, C.byref(w), C.byref(h)))
        out = np.zeros((h.value + 2 * border, w.value + 2 * border), np.uint8)
        _check(self.L.aos2_extractor_pyramid_level(self.h, image, level, border, _p(out), out.strides[0]))
        return out

    def debug_candidates(self, level, image=0):
        n = C.c_int(0)
        _check(self.L.aos2_extractor_debug_candidates(self.h, image, level, None, None, None, 0, C.byref(n)))
        xs = np.zeros(max(n.value, 1), np.int16)
        ys = np.zeros(max(n.value, 1), np.int16)
        sc = np.zeros(max(n.value, 1), np.uint8)
        _check(self.L.aos2_extractor_debug_candidates(self.h, image, level, _p(xs), _p(ys), _p(sc), len(xs), C.byref(n)))
        return xs[: n.value], ys[: n.value], sc[: n.value]

    def debug_plan(self, w, h):
        """aos2_debug_extractor_plan: the plan for w x h images, computed on the host (no device) -> dict(levels int64 [nlevels][4] =
        w, h, pitch, off; cells int32 [n][6] = level, vx0, vy0, cw, ch, slot_off; pyr_bytes; slot_total)"""
        levels, totals, n = np.zeros((self.nlevels, 4), np.int64), np.zeros(2, np.int64), C.c_int(0)
        _check(self.L.aos2_debug_extractor_plan(self.h, int(w), int(h), _p(levels), None, 0, C.byref(n), _p(totals)))
        cells = np.zeros((max(n.value, 1), 6), np.int32)
        _check(self.L.aos2_debug_extractor_plan(self.h, int(w), int(h), _p(levels), _p(cells), len(cells), C.byref(n), _p(totals)))
        return dict(levels=levels, cells=cells[: n.value], pyr_bytes=int(totals[0]), slot_total=int(totals[1]))

    def set_chunks(self, n):
        _check(self.L.aos2_extractor_set_chunks(self.h, n))

    def last_timing(self):
        t = np.zeros(8, np.float32)
        _check(self.L.aos2_extractor_last_timing(self.h, _p(t), 8))
        return dict(pyramid=float(t[0]), fast=float(t[1]), compact=float(t[2]), octree=float(t[3]),
                    describe=float(t[4]), total_wall=float(t[5]), chunks=int(t[6]))

    def bench_fast(self, iters=20):
        ms = C.c_float(0)
        _check(self.L.aos2_extractor_bench_fast(self.h, iters, C.byref(ms)))
        return ms.value

    def bench_describe(self, iters=20):
        ms = C.c_float(0)
        _check(self.L.aos2_extractor_bench_describe(self.h, iters, C.byref(ms)))
        return ms.value


class Vocabulary(_Handle):
    """ORBVocabulary (include/ORBVocabulary.h:31-32): loaders, transform(), score()."""

    KIND = "vocabulary"

    def __init__(self, device=0):
        self._create(device)

    def loadFromBinaryFile(self, path):
        return self.L.aos2_vocabulary_load_binary(self.h, str(path).encode()) == AOS2_OK

    def loadFromTextFile(self, path):
        return self.L.aos2_vocabulary_load_text(self.h, str(path).encode()) == AOS2_OK

    def saveToBinaryFile(self, path):
        _check(self.L.aos2_vocabulary_save_binary(self.h, str(path).encode()))

    def set_nodes(self, k, L, scoring, weighting, parent, desc, weight, is_leaf):
        parent = np.ascontiguousarray(parent, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8)
        weight = np.ascontiguousarray(weight, np.float64)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        _check(self.L.aos2_vocabulary_set_nodes(self.h, k, L, scoring, weighting, len(parent), _p(parent), _p(desc),
                                                _p(weight), _p(is_leaf)))

    def info(self):
        g = lambda n: getattr(self.L, "aos2_vocabulary_" + n)(self.h)  # noqa: E731
        return dict(k=g("k"), L=g("levels"), scoring=g("scoring"), weighting=g("weighting"), nodes=g("nodes"),
                    words=int(g("size")))

    def nodes(self):
        """m_nodes, root included -> dict(parent, is_leaf (= no children), word_id, weight, desc)"""
        n = self.L.aos2_vocabulary_nodes(self.h)
        r = dict(parent=np.zeros(n, np.int32), is_leaf=np.zeros(n, np.uint8), word_id=np.zeros(n, np.uint32),
                 weight=np.zeros(n, np.float64), desc=np.zeros((n, 32), np.uint8))
        _check(self.L.aos2_vocabulary_get_nodes(self.h, *[_p(r[k]) for k in ("parent", "is_leaf", "word_id", "weight", "desc")]))
        return r

    def empty(self):
        return bool(self.L.aos2_vocabulary_empty(self.h))

    def transform(self, desc, levelsup=4):
        """-> dict(bow_word, bow_value, fv_node, fv_off, fv_idx, word_of, node_of)"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        bw, bv = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fn, fo, fi = np.zeros(m, np.int32), np.zeros(n + 2, np.int32), np.zeros(m, np.int32)
        wo, no = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        nb, nf = C.c_int(0), C.c_int(0)
        _check(self.L.aos2_vocabulary_transform(self.h, _p(desc), n, levelsup, _p(bw), _p(bv), C.byref(nb), _p(fn), _p(fo),
                                                _p(fi), C.byref(nf), _p(wo), _p(no)))
        nb, nf = nb.value, nf.value
        return dict(bow_word=bw[:nb].copy(), bow_value=bv[:nb].copy(), fv_node=fn[:nf].copy(), fv_off=fo[: nf + 1].copy(),
                    fv_idx=fi[: fo[nf]].copy(), word_of=wo[:n].copy(), node_of=no[:n].copy())

    def transform_device(self, batch, d_desc, d_n, cap, levelsup, d_bw, d_bv, d_nb, d_fn, d_fo, d_fi, d_nf, d_wo=0, d_no=0):
        """raw device pointers (ints); returns the device time in ms"""
        V = C.c_void_p
        _check(self.L.aos2_vocabulary_transform_device(self.h, batch, V(d_desc), V(d_n), cap, levelsup, V(d_bw), V(d_bv),
                                                       V(d_nb), V(d_fn), V(d_fo), V(d_fi), V(d_nf), V(d_wo or None),
                                                       V(d_no or None)))
        return float(self.L.aos2_vocabulary_last_device_ms(self.h))

    def stream(self):
        return self.L.aos2_vocabulary_stream(self.h)

    def score(self, a, b):
        w1, v1 = np.ascontiguousarray(a["bow_word"], np.uint32), np.ascontiguousarray(a["bow_value"], np.float64)
        w2, v2 = np.ascontiguousarray(b["bow_word"], np.uint32), np.ascontiguousarray(b["bow_value"], np.float64)
        s = C.c_double(0)
        _check(self.L.aos2_vocabulary_score(self.h, _p(w1), _p(v1), len(w1), _p(w2), _p(v2), len(w2), C.byref(s)))
        return s.value


def ComputeStereoMatches(left: Extractor, right: Extractor, kps_l, desc_l, kps_r, desc_r, mb, mbf, image=0):
    """Frame::ComputeStereoMatches (src/Frame.cc:495-669) on the pyramids `left` / `right` hold from their
    last extract.  Returns (mvuRight, mvDepth) float32 arrays, -1 = no match."""
    kps_l = np.ascontiguousarray(kps_l, KP_DTYPE)
    kps_r = np.ascontiguousarray(kps_r, KP_DTYPE)
    desc_l = np.ascontiguousarray(desc_l, np.uint8)
    desc_r = np.ascontiguousarray(desc_r, np.uint8)
    ur = np.full(len(kps_l), -1.0, np.float32)
    dp = np.full(len(kps_l), -1.0, np.float32)
    _check(left.L.aos2_compute_stereo_matches(left.h, right.h, image, _p(kps_l), _p(desc_l), len(kps_l), _p(kps_r),
                                              _p(desc_r), len(kps_r), mb, mbf, _p(ur), _p(dp)))
    return ur, dp


def compute_stereo_matches_device(left: Extractor, right: Extractor, batch, d_kpl, d_dl, d_nl, d_kpr, d_dr, d_nr, cap,
                                  mb, mbf, d_ur, d_depth):
    """raw device pointers (ints); arrays as written by extract_batch_device for the two eyes"""
    V = C.c_void_p
    _check(left.L.aos2_compute_stereo_matches_device(left.h, right.h, batch, V(d_kpl), V(d_dl), V(d_nl), V(d_kpr),
                                                     V(d_dr), V(d_nr), cap, mb, mbf, V(d_ur), V(d_depth)))
    return float(left.L.aos2_compute_stereo_matches_last_device_ms(left.h))


def compute_stereo_matches_device_async(left: Extractor, right: Extractor, batch, d_kpl, d_dl, d_nl, d_kpr, d_dr, d_nr, cap,
                                        mb, mbf, d_ur, d_depth):
    """the same, enqueued behind both extractors' batches in flight (no host wait)"""
    V = C.c_void_p
    _check(left.L.aos2_compute_stereo_matches_device_async(left.h, right.h, batch, V(d_kpl), V(d_dl), V(d_nl), V(d_kpr),
                                                           V(d_dr), V(d_nr), cap, mb, mbf, V(d_ur), V(d_depth)))
