/*
 * aos2.h -- C ABI of the MI355X-native ORB front-end + LocalBA hot path.
 *
 * This is the drop-in boundary under the reference's three C++ class surfaces
 * (SURVEY.md section 8(b)); every entry point names the reference interface it replaces
 * (path:line relative to the Active-ORB-SLAM2 checkout).  Plain C, POD arguments, caller-allocated
 * buffers, int status (0 = ok, <0 = error, see AOS2_ERR_*).  No torch / OpenCV / Eigen types.
 *
 * Threading: a handle is NOT re-entrant (like an ORBextractor instance, which owns a mutable
 * mvImagePyramid); different handles may be used concurrently from different threads (the stereo
 * path runs one extractor per eye, src/Frame.cc:103-106).  Each handle owns one HIP stream.
 *
 * There is no CPU fallback: every compute entry point returns AOS2_ERR_NO_DEVICE when no HIP
 * device is present.
 */
#ifndef AOS2_H
#define AOS2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOS2_OK 0
#define AOS2_ERR_ARG (-1)        /* bad argument (NULL, non-positive size, unsupported layout) */
#define AOS2_ERR_CAPACITY (-2)   /* output buffer too small; *n_out still holds the needed count */
#define AOS2_ERR_TOO_SMALL (-3)  /* image too small for the pyramid (reference would divide by 0) */
#define AOS2_ERR_HIP (-4)        /* HIP runtime error, see aos2_last_error() */
#define AOS2_ERR_NO_DEVICE (-5)  /* no HIP device / device index out of range */
#define AOS2_ERR_STOPPED (1)     /* LocalBA: stop flag was set before optimisation started */

/* last error text of the calling thread */
const char *aos2_last_error(void);
/* number of HIP devices visible (0 when none; never fails) */
int aos2_device_count(void);
const char *aos2_version(void);
/* The host CPUs local to the device (the NUMA node its PCIe root hangs off), as the kernel's list string ("0-63,128-191": sysfs
 * local_cpulist of the device's PCI function); "" when the platform does not say.  For callers that place their threads: bench.py's
 * composite ran at 51-52 k frames/s when pinned to the other socket's CPUs and at 59-63 k on the local ones (AOS2_BENCH_NUMA; on the
 * shared hosts of the test pool the unpinned default was as good as the local node).  Returns AOS2_ERR_CAPACITY
 * when `cap` is too small, AOS2_ERR_NO_DEVICE without that device.  No reference equivalent (the reference never leaves the CPU). */
int aos2_device_local_cpus(int device, char *buf, int cap);

/* ------------------------------------------------------------------------------------------
 * ORBextractor  (include/ORBextractor.h:45-111, src/ORBextractor.cc)
 * ------------------------------------------------------------------------------------------ */

/* bit-compatible with cv::KeyPoint (28 bytes) */
typedef struct {
    float x, y;      /* pt, level-0 pixel units */
    float size;      /* 31 * scale[octave], truncated (src/ORBextractor.cc:837,846) */
    float angle;     /* degrees [0,360) */
    float response;  /* FAST-9/16 corner score */
    int32_t octave;
    int32_t class_id; /* -1 */
} aos2_keypoint_t;

typedef struct aos2_extractor aos2_extractor_t;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * src/ORBextractor.cc:410-470.  device = HIP device index.  Creation only builds the host-side
 * tables (no HIP call), so it succeeds without a GPU; the first extract binds the device. */
int aos2_extractor_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast,
                          int min_th_fast, int device, aos2_extractor_t **out);
void aos2_extractor_destroy(aos2_extractor_t *e);

/* GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:58-83).  Arrays have nlevels entries and
 * live as long as the handle. */
int aos2_extractor_levels(const aos2_extractor_t *e);
float aos2_extractor_scale_factor(const aos2_extractor_t *e);
const float *aos2_extractor_scale_factors(const aos2_extractor_t *e);
const float *aos2_extractor_inv_scale_factors(const aos2_extractor_t *e);
const float *aos2_extractor_sigma2(const aos2_extractor_t *e);
const float *aos2_extractor_inv_sigma2(const aos2_extractor_t *e);
/* mnFeaturesPerLevel (include/ORBextractor.h:101) and umax (:103) -- exposed for tests */
const int *aos2_extractor_features_per_level(const aos2_extractor_t *e);
const int *aos2_extractor_umax(const aos2_extractor_t *e);

/* ORBextractor::operator()(image, mask, keypoints, descriptors)  src/ORBextractor.cc:1043-1105.
 * img: 8-bit single channel, host memory, `stride` bytes per row (the CV_8UC1 assert of :1050 is
 * the caller's contract).  mask is ignored by the reference and has no parameter here.
 * kps[cap], desc[cap*32] are caller-allocated (host).  *n_out = number of keypoints.
 * Empty image (img==NULL or w<=0 or h<=0) -> AOS2_OK with *n_out = 0 (silent return, :1046).
 * The result can exceed nfeatures by a few keypoints (octree overshoot);
 * cap >= aos2_extractor_max_keypoints() always suffices. */
int aos2_extractor_extract(aos2_extractor_t *e, const uint8_t *img, int w, int h, int stride,
                           aos2_keypoint_t *kps, uint8_t *desc, int cap, int *n_out);
int aos2_extractor_max_keypoints(const aos2_extractor_t *e);
/* The same bound for a given image size, before any image was seen: DistributeOctTree's first pass divides all
 * round(W / H) root nodes (src/ORBextractor.cc:549-590), so a wide image with few features per level can return more
 * than nfeatures-per-level + 3 keypoints (4 * round(W / H) per level). */
int aos2_extractor_max_keypoints_for(const aos2_extractor_t *e, int w, int h);

/* Batched form for frame-parallel throughput: `batch` images of identical size, host memory,
 * image b at imgs + b*image_stride.  Outputs are [batch][cap] / [batch][cap][32] / [batch]. */
int aos2_extractor_extract_batch(aos2_extractor_t *e, const uint8_t *imgs, int batch, int w, int h,
                                 int stride, size_t image_stride, aos2_keypoint_t *kps,
                                 uint8_t *desc, int cap, int32_t *n_out);

/* Page-locked host memory for the host-pointer entry points above.  Optional: any host memory works.  The batched
 * call uploads, computes and downloads chunk by chunk on separate streams, so the PCIe copies of one part of the
 * batch overlap the kernels of another; page-locked RESULT buffers matter most (256 TUM frames: 2.1 ms per call =
 * 120 k frames/s, 44 GB/s over PCIe, against 8.8 ms with the un-pipelined copies into pageable results this replaced;
 * pageable and page-locked INPUTS measured the same, tools/gpu_latency.py).  AOS2_ERR_NO_DEVICE without a GPU. */
int aos2_host_alloc(void **p, size_t bytes);
int aos2_host_free(void *p);

/* Same with inputs and outputs resident in device memory (HBM).  d_* are device pointers owned
 * by the caller; the call is synchronous on the handle's stream (returns when results are in
 * d_kps / d_desc / d_n_out). */
int aos2_extractor_extract_batch_device(aos2_extractor_t *e, const uint8_t *d_imgs, int batch,
                                        int w, int h, int stride, size_t image_stride,
                                        aos2_keypoint_t *d_kps, uint8_t *d_desc, int cap,
                                        int32_t *d_n_out);

/* Asynchronous form of the above: enqueues the batch on the handle's HIP streams and returns; the outputs are
 * complete, and errors (octree capacity, more keypoints than `cap`) reported, by aos2_extractor_wait().
 * Several batches may be enqueued before one wait: chunk c of every batch runs on stream c with its own scratch,
 * so the latency-bound octree stage of one batch overlaps the FAST / descriptor kernels of the next (the
 * frame-parallel pipeline of SURVEY.md section 8(e)).  The caller must not reuse the input or output buffers of a
 * batch that is still in flight, and all batches of one flight share (w, h, cap, batch); a change of geometry or
 * of batch size waits for the flight first.  Every other call on the handle waits for the flight implicitly. */
int aos2_extractor_extract_batch_device_async(aos2_extractor_t *e, const uint8_t *d_imgs, int batch,
                                              int w, int h, int stride, size_t image_stride,
                                              aos2_keypoint_t *d_kps, uint8_t *d_desc, int cap,
                                              int32_t *d_n_out);
int aos2_extractor_wait(aos2_extractor_t *e);
/* Device-side ordering instead of a host wait: everything enqueued on `hip_stream` (a hipStream_t of the caller, e.g.
 * the stream of an aos2_frames_t, or 0 for the null stream) after this call runs after everything enqueued on the
 * extractor's streams before it.  Errors of the batches in flight are still reported by aos2_extractor_wait(). */
int aos2_extractor_stream_wait(aos2_extractor_t *e, void *hip_stream);
/* The other direction: every batch enqueued on the extractor after this call runs after everything enqueued on `hip_stream` before
 * it -- e.g. the caller's own hipMemcpyAsync of the images from page-locked host memory (the reference's images arrive as host
 * cv::Mat, src/Frame.cc:276-282; bench.py --host-images).  Device-side, no host wait. */
int aos2_extractor_wait_for_stream(aos2_extractor_t *e, void *hip_stream);
/* The exchange step of the frame-sharded path: packs the device outputs of a batch into fixed-size
 * per-frame slots {int32 n; int32 pad[3]; KeyPoint[cap]; uint8 desc[cap][32]} (slot_bytes each, a multiple of 16, unused
 * tail zeroed) that one collective (RCCL gather over xGMI) moves to rank 0.  Enqueued on `hip_stream` behind the
 * extractor's pending work; cap must be a multiple of 4. */
int aos2_extractor_pack_slots(aos2_extractor_t *e, int batch, const aos2_keypoint_t *d_kps, const uint8_t *d_desc,
                              const int32_t *d_n, int cap, uint8_t *d_slots, size_t slot_bytes, void *hip_stream);

/* mvImagePyramid[level] (include/ORBextractor.h:85; read by Frame::ComputeStereoMatches,
 * src/Frame.cc:502,592,609) of image `image` of the last extract on this handle.
 * Copies the level to host memory `dst` with row pitch dst_stride.  border = 0 gives the w x h
 * interior (the ROI the reference exposes); border = 19 gives the (w+38) x (h+38) buffer with the
 * BORDER_REFLECT_101 frame the reference keeps around it (:1113-1128). */
int aos2_extractor_pyramid_level_size(const aos2_extractor_t *e, int level, int *w, int *h);
int aos2_extractor_pyramid_level(aos2_extractor_t *e, int image, int level, int border,
                                 uint8_t *dst, int dst_stride);

/* Frame::ComputeStereoMatches()  src/Frame.cc:495-669  (SURVEY.md §8(f) rank 2).
 * `left` / `right` are the two ORBextractor handles of the stereo Frame (mpORBextractorLeft / Right,
 * include/Frame.h:108); both must still hold the device pyramids of their last extract*() call
 * (mvImagePyramid, read at :502,592,609) and `image` selects the image of that batch.
 * kp_* / desc_* = mvKeys / mvKeysRight and mDescriptors / mDescriptorsRight (host memory).
 * mb = baseline in metres (minZ, :526), mbf = baseline * fx (:527).
 * Outputs mvuRight[n_left], mvDepth[n_left]; -1 = no stereo match (:498).
 * When no left keypoint passes the SAD stage the reference reads vDistIdx[0] of an empty vector
 * (:655); here that case leaves every output at -1.
 * Domain of ComputeStereoMatches.  With (w_l, h_l) the size of mvImagePyramid[l], inv = mvInvScaleFactors and round()
 * half away from zero:
 *   left keypoint:  0 <= octave < nlevels; x, y finite; 0 <= (int)y < rows of level 0;
 *                   5 <= round(x * inv[octave]) <= w_octave - 6 and 5 <= round(y * inv[octave]) <= h_octave - 6;
 *   right keypoint: 0 <= octave < nlevels; y finite; for every existing level l in octave-1 .. octave+1,
 *                   round(x * inv[l]) is negative (refused by iniu < 0, :604) or at least 10.
 * Inside it the 11 x 11 left window (:592) and the 11 x 21 right window (:609) stay inside the level; outside it the
 * reference throws from rowRange / colRange.  Every keypoint the extractor writes is inside it.  This call checks the
 * records on the host and returns AOS2_ERR_ARG, with the outputs untouched and nothing uploaded or launched, when one is
 * outside. */
int aos2_compute_stereo_matches(aos2_extractor_t *left, aos2_extractor_t *right, int image,
                                const aos2_keypoint_t *kp_left, const uint8_t *desc_left, int n_left,
                                const aos2_keypoint_t *kp_right, const uint8_t *desc_right,
                                int n_right, float mb, float mbf, float *u_right, float *depth);
/* Batched, fully device-resident form: the arrays are exactly what
 * aos2_extractor_extract_batch_device() wrote for the two eyes ([batch][cap] keypoints,
 * [batch][cap][32] descriptors, [batch] counts; descriptor blocks 16-byte aligned); image b of the
 * call = image b of both extractors' last batch.  d_u_right / d_depth are [batch][cap].
 * Precondition: every record lies in the domain above.  The device-resident forms cannot look at the records and do not
 * check it; arrays written by aos2_extractor_extract_batch_device() satisfy it, anything else is the caller's to verify. */
int aos2_compute_stereo_matches_device(aos2_extractor_t *left, aos2_extractor_t *right, int batch,
                                       const aos2_keypoint_t *d_kp_left, const uint8_t *d_desc_left,
                                       const int32_t *d_n_left, const aos2_keypoint_t *d_kp_right,
                                       const uint8_t *d_desc_right, const int32_t *d_n_right,
                                       int cap, float mb, float mbf, float *d_u_right, float *d_depth);
/* The same without a host wait: left's first stream waits on the device for both extractors' batches in flight
 * (aos2_extractor_extract_batch_device_async -- the two ExtractORB threads of src/Frame.cc:103-109 joined), the kernels
 * are enqueued behind; what orders itself behind `left` afterwards (aos2_extractor_stream_wait, aos2_frames_build_stereo,
 * aos2_extractor_wait) runs behind them.  The kernels read BOTH extractors' pyramid blocks: the next extraction of either
 * extractor waits for them on the device, on every stream it uses, before it rewrites the pyramids -- the calls can be
 * pipelined without a host wait in between.  The keypoint / descriptor / count / output buffers of the call are the
 * caller's to keep untouched until left's stream has drained.  No device time is recorded.
 * An extractor is paired with one partner at a time: pairing either eye with a third extractor ends the earlier pairing.  The
 * ordering above is kept for calls that were executed; for a call that was RECORDED (aos2_capture_begin) with the earlier
 * partner it ends there, so wait for the replays of such a recording before that partner extracts again. */
int aos2_compute_stereo_matches_device_async(aos2_extractor_t *left, aos2_extractor_t *right, int batch,
                                             const aos2_keypoint_t *d_kp_left, const uint8_t *d_desc_left,
                                             const int32_t *d_n_left, const aos2_keypoint_t *d_kp_right,
                                             const uint8_t *d_desc_right, const int32_t *d_n_right,
                                             int cap, float mb, float mbf, float *d_u_right, float *d_depth);
/* device time (ms) of the kernels of the last ComputeStereoMatches call on `left` */
float aos2_compute_stereo_matches_last_device_ms(const aos2_extractor_t *left);

/* Stage taps for parity tests (no reference equivalent): FAST candidates handed to
 * DistributeOctTree for (image, level) of the last extract, in the reference's emission order
 * (cells row-major, pixels row-major inside a cell); coordinates relative to (minBorderX,
 * minBorderY) like src/ORBextractor.cc:822-823. Returns count via *n (arrays may be NULL). */
int aos2_extractor_debug_candidates(aos2_extractor_t *e, int image, int level, int16_t *xs,
                                    int16_t *ys, uint8_t *score, int cap, int *n);

/* A batch is cut into `chunks` sub-batches that run on separate HIP streams so that the
 * latency-bound octree kernel of one overlaps the streaming kernels of the others.
 * 0 = automatic (2 for batch >= 64, else 1); 1 = one stream (stage timing below is
 * only meaningful then); at most 4. */
int aos2_extractor_set_chunks(aos2_extractor_t *e, int chunks);

/* Timing of the last batch, milliseconds, measured with HIP events on the handle's stream:
 * [0] pyramid kernels, [1] FAST+NMS kernel, [2] empty (two back-to-back events: the slot of a
 * former candidate compaction stage, kept so the layout stays), [3] octree kernel, [4] orientation +
 * blur + rBRIEF kernel, [5] whole call (host wall clock).  n <= 8 values are written. */
int aos2_extractor_last_timing(const aos2_extractor_t *e, float *ms, int n);

/* Launches only the FAST+NMS kernel `iters` times on the pyramid of the last batch and returns
 * the average kernel time in ms (HIP events on the handle's stream) -- roofline measurement. */
int aos2_extractor_bench_fast(aos2_extractor_t *e, int iters, float *avg_ms);
int aos2_extractor_bench_describe(aos2_extractor_t *e, int iters, float *avg_ms);

/* ------------------------------------------------------------------------------------------
 * ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>   
 * (include/ORBVocabulary.h:31-32, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h)
 * ------------------------------------------------------------------------------------------ */
typedef struct aos2_vocabulary aos2_vocabulary_t;

/* DBoW2 enums (Thirdparty/DBoW2/DBoW2/BowVector.h:36-53) */
#define AOS2_WEIGHT_TF_IDF 0
#define AOS2_WEIGHT_TF 1
#define AOS2_WEIGHT_IDF 2
#define AOS2_WEIGHT_BINARY 3
#define AOS2_SCORING_L1_NORM 0
#define AOS2_SCORING_L2_NORM 1
#define AOS2_SCORING_CHI_SQUARE 2
#define AOS2_SCORING_KL 3
#define AOS2_SCORING_BHATTACHARYYA 4
#define AOS2_SCORING_DOT_PRODUCT 5

int aos2_vocabulary_create(int device, aos2_vocabulary_t **out);
void aos2_vocabulary_destroy(aos2_vocabulary_t *v);
/* bool loadFromBinaryFile(filename) :1456-1496 / loadFromTextFile :1351-1431 (src/System.cc:89-92),
 * saveToBinaryFile :1500-1521.  Both loaders reproduce the reference's `while(!f.eof())` tail
 * (binary: the last record is appended twice; text: a final newline yields one more, childless,
 * zero-weight child of the root, counted as a word) -- see DESIGN.md §5.5.  A text header the reference refuses
 * leaves the vocabulary empty with k and L taken from that header. */
int aos2_vocabulary_load_binary(aos2_vocabulary_t *v, const char *filename);
int aos2_vocabulary_load_text(aos2_vocabulary_t *v, const char *filename);
int aos2_vocabulary_save_binary(const aos2_vocabulary_t *v, const char *filename);
/* Programmatic construction (no reference equivalent; the vocabulary file is absent):
 * record i describes node i+1 exactly like one record of the binary file (parent id, 32-byte
 * descriptor, weight, leaf flag); parents must precede their children. */
int aos2_vocabulary_set_nodes(aos2_vocabulary_t *v, int k, int L, int scoring, int weighting,
                              int n_nodes, const int32_t *parent, const uint8_t *desc,
                              const double *weight, const uint8_t *is_leaf);
int aos2_vocabulary_k(const aos2_vocabulary_t *v);          /* getBranchingFactor() */
int aos2_vocabulary_levels(const aos2_vocabulary_t *v);     /* getDepthLevels() */
int aos2_vocabulary_scoring(const aos2_vocabulary_t *v);    /* getScoringType() */
int aos2_vocabulary_weighting(const aos2_vocabulary_t *v);  /* getWeightingType() */
int aos2_vocabulary_nodes(const aos2_vocabulary_t *v);      /* m_nodes.size() */
unsigned aos2_vocabulary_size(const aos2_vocabulary_t *v);  /* size() = number of words */
int aos2_vocabulary_empty(const aos2_vocabulary_t *v);      /* empty() */
/* Read-only view of m_nodes, root (node 0) included: aos2_vocabulary_nodes() entries each of parent, isLeaf() (no children),
 * word id, weight and 32 descriptor bytes.  Any pointer may be NULL. */
int aos2_vocabulary_get_nodes(const aos2_vocabulary_t *v, int32_t *parent, uint8_t *is_leaf, uint32_t *word_id,
                              double *weight, uint8_t *desc);

/* void transform(const vector<TDescriptor>& features, BowVector&, FeatureVector&, int levelsup)
 * :1140-1187 (Frame::ComputeBoW src/Frame.cc:424-431 and KeyFrame::ComputeBoW call it with
 * levelsup = 4).  desc: n x 32 bytes, host.  The two std::maps are returned as key-ascending arrays:
 *   BowVector     bow_word[*n_bow], bow_value[*n_bow]                       (capacity n each)
 *   FeatureVector fv_node[*n_fv], fv_off[*n_fv + 1], fv_idx[fv_off[*n_fv]]  (capacity n, n+1, n)
 * -- the CSR layout aos2_bow_pair_t takes.  word_of / node_of (optional, n each): per-feature word id
 * and node id at level L - levelsup (transform(feature, id, weight, &nid, levelsup) :1215-1260).
 * An empty vocabulary clears both outputs and returns AOS2_OK (:1147-1150). */
int aos2_vocabulary_transform(aos2_vocabulary_t *v, const uint8_t *desc, int n, int levelsup,
                              uint32_t *bow_word, double *bow_value, int *n_bow, int32_t *fv_node,
                              int32_t *fv_off, int32_t *fv_idx, int *n_fv, uint32_t *word_of,
                              uint32_t *node_of);
/* Batched device-resident form: d_desc [batch][cap][32] and d_n [batch] as written by
 * aos2_extractor_extract_batch_device; outputs [batch][cap] (d_fv_off: [batch][cap + 1]),
 * counts [batch].  d_word_of / d_node_of may be NULL.  cap <= 8192. */
int aos2_vocabulary_transform_device(aos2_vocabulary_t *v, int batch, const uint8_t *d_desc,
                                     const int32_t *d_n, int cap, int levelsup,
                                     uint32_t *d_bow_word, double *d_bow_value, int32_t *d_n_bow,
                                     int32_t *d_fv_node, int32_t *d_fv_off, int32_t *d_fv_idx,
                                     int32_t *d_n_fv, uint32_t *d_word_of, uint32_t *d_node_of);
float aos2_vocabulary_last_device_ms(const aos2_vocabulary_t *v);
/* the handle's hipStream_t (the transforms run on it): lets a caller order a transform behind the producer of d_desc on
 * the device, e.g. aos2_extractor_stream_wait(e, aos2_vocabulary_stream(v)) after enqueuing the extraction */
void *aos2_vocabulary_stream(aos2_vocabulary_t *v);
/* double score(const BowVector&, const BowVector&) :1191-1195 for L1_NORM
 * (L1Scoring::score, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-72); host scalar helper. */
int aos2_vocabulary_score(const aos2_vocabulary_t *v, const uint32_t *w1, const double *v1, int n1,
                          const uint32_t *w2, const double *v2, int n2, double *score);

/* ------------------------------------------------------------------------------------------
 * KeyFrameDatabase  (include/KeyFrameDatabase.h:42-70, src/KeyFrameDatabase.cc)
 * The step in front of Tracking::Relocalization (src/Tracking.cc:1528) and LoopClosing::ComputeSim3 (src/LoopClosing.cc:143):
 * which keyframes they work on.  A database holds SLOTS: a slot is a keyframe's BowVector (word ids ascending, double values)
 * resident in HBM.  A slot is PUT when the keyframe gets its BowVector, ADDED by add(), ERASED by erase() (it leaves the
 * queries and keeps its BowVector) and DROPPED when its row is freed.  There is no limit on keyframes or on words per keyframe.
 * DESIGN.md section 2 item 13 (reloc_score, "shares a word"), section 4 (layout), section 5 (kernels).
 * ------------------------------------------------------------------------------------------ */
typedef struct aos2_kfdb aos2_kfdb_t;
#define AOS2_KFDB_LOOP 0          /* DetectLoopCandidates           src/KeyFrameDatabase.cc:76-197 */
#define AOS2_KFDB_RELOC 1         /* DetectRelocalizationCandidates :199-309 */
#define AOS2_KFDB_NEIGHBOURS 10   /* GetBestCovisibilityKeyFrames(10) :151, :265 */

/* KeyFrameDatabase(const ORBVocabulary&) :33-37: the scoring type (only L1_NORM, as aos2_vocabulary_score; anything else is
 * AOS2_ERR_ARG) and the word count (mvInvertedFile.resize(voc.size())) are taken from `voc`, which is not kept. */
int aos2_kfdb_create(const aos2_vocabulary_t *voc, int device, aos2_kfdb_t **out);
void aos2_kfdb_destroy(aos2_kfdb_t *db);
/* pKF->mBowVec of a new keyframe (KeyFrame::ComputeBoW): n >= 0 words, ids ascending without repeats and below the vocabulary's
 * word count (else AOS2_ERR_ARG).  *slot = the new slot; reloc_score = 0.0f, no neighbours, not added.  Needs no device. */
int aos2_kfdb_put(aos2_kfdb_t *db, const uint32_t *words, const double *values, int n, int32_t *slot);
/* `batch` rows as aos2_vocabulary_transform_device wrote them (d_words / d_values [batch][cap], d_n_bow [batch]), ordered behind
 * the stream of `voc` (may be NULL: the caller has waited).  slots [batch]. */
int aos2_kfdb_put_device(aos2_kfdb_t *db, aos2_vocabulary_t *voc, int batch, const uint32_t *d_words, const double *d_values,
                         const int32_t *d_n_bow, int cap, int32_t *slots);
/* add(KeyFrame*) :40-46: the slot takes the next value of a 64-bit add counter (its place in every inverted list).  Adding an
 * added slot is AOS2_ERR_ARG (the reference never does it and would count the keyframe twice). */
int aos2_kfdb_add(aos2_kfdb_t *db, int32_t slot);
/* erase(KeyFrame*) :48-67; erasing a slot that is not added does nothing, as there */
int aos2_kfdb_erase(aos2_kfdb_t *db, int32_t slot);
/* frees the row (~KeyFrame); an added slot is erased first.  The slot number may be handed out again. */
int aos2_kfdb_drop(aos2_kfdb_t *db, int32_t slot);
/* clear() :69-73: un-adds everything; the slots stay put */
int aos2_kfdb_clear(aos2_kfdb_t *db);
int aos2_kfdb_size(const aos2_kfdb_t *db);             /* number of added slots */
int64_t aos2_kfdb_arena_capacity(const aos2_kfdb_t *db);   /* entries the device arena holds now (0 before the first device call) */
/* GetBestCovisibilityKeyFrames(10) of n slots: neigh [n][10] slot numbers in that order, -1 padded.  Resident: the caller
 * refreshes the rows it changes.  A neighbour that is not put (or dropped later) takes no part. */
int aos2_kfdb_set_neighbours(aos2_kfdb_t *db, int n, const int32_t *slots, const int32_t *neigh);

typedef struct {
    int32_t mode;             /* AOS2_KFDB_LOOP / AOS2_KFDB_RELOC */
    int32_t slot;             /* >= 0: the query is this slot's BowVector (put is enough); < 0: words / values */
    const uint32_t *words;    /* [n_words] ascending;  host arrays, or device arrays with on_device = 1 */
    const double *values;
    int32_t n_words;
    int32_t on_device;
    float min_score;          /* LOOP: minScore (:76) */
    int32_t n_excluded;       /* LOOP: spConnectedKeyFrames (:78) as slots, host; entries that are not added are ignored */
    const int32_t *excluded;
} aos2_kfdb_query_t;

typedef struct {
    int32_t *candidates;      /* vpLoopCandidates :179-196 / vpRelocCandidates :292-308, in order; caller-allocated [cap_candidates] */
    int32_t cap_candidates;
    int32_t n_candidates;
    int32_t n_sharing;        /* lKFsSharingWords.size() :107 / :224 */
    int32_t max_common_words; /* :113-118 / :228-233 */
    int32_t min_common_words; /* (int)(maxCommonWords * 0.8f) :120 / :235 */
    int32_t n_scored;         /* nscores :131 / :248 */
    int32_t n_matched;        /* lScoreAndMatch.size() :141 / :255 */
    float best_acc_score;     /* bestAccScore :145-173 / :259-287 (its start value when nothing is matched) */
    /* optional (NULL: not wanted), in list order.  The scored list: the slots with words > minCommonWords (:129 / :246) */
    int32_t *scored_slot, *scored_words;
    float *scored_score;
    int32_t cap_scored;
    /* the sharing list lKFsSharingWords with mnLoopWords / mnRelocWords */
    int32_t *sharing_slot, *sharing_words;
    int32_t cap_sharing;
} aos2_kfdb_result_t;

/* DetectLoopCandidates :76-197 / DetectRelocalizationCandidates :199-309 for nq queries in one call.  The RELOC queries of a
 * call take effect on reloc_score (mRelocScore :250, read at :276) in index order.  nq == 0 and an empty database are AOS2_OK.
 * AOS2_ERR_ARG (a NULL, a bad mode, a slot that is not put, a negative count or capacity, query words that do not ascend) is
 * reported before anything runs and leaves every result byte as it was.  AOS2_ERR_CAPACITY: a list did not fit; the counts
 * hold what is needed, the lists are filled up to their capacities, and reloc_score has been updated. */
int aos2_kfdb_detect(aos2_kfdb_t *db, const aos2_kfdb_query_t *queries, aos2_kfdb_result_t *results, int nq);
/* The loop of LoopClosing::DetectLoop (src/LoopClosing.cc:126-140): scores [n] = (float) score(query, slots[i]) (put is enough)
 * and *min_score = their minimum starting from 1.  mode, min_score and excluded of the query are not read. */
int aos2_kfdb_scores(aos2_kfdb_t *db, const aos2_kfdb_query_t *query, const int32_t *slots, int n, float *scores,
                     float *min_score);
float aos2_kfdb_last_device_ms(const aos2_kfdb_t *db);   /* device time of the last detect / scores call (HIP events) */

/* ------------------------------------------------------------------------------------------
 * camera (planner visibility)  (include/camera.h:51-129, src/camera.cc)
 * What the Active-SLAM planner asks of every robot state it tries: how many points of the whole map are predicted to be visible
 * from it (camera::countVisible :135-198 over camera::isInFrustum :263-315).  The reference answers one state per call, serially,
 * from StateValidChecker::isValid / checkMotion (src/StateValidChecker.cc:97-161), MotionCostCamera (:531-541),
 * plan_slam::AdvanceStepCamera (src/plan.cc:141-151) and RRTstar::display_costs (src/myRRTstar.cc:1142-1163); here a call takes
 * a batch of states against a map resident in HBM.  Every output equals the serial loop bit for bit, the float sum included
 * (DESIGN.md section 2 item 16, section 5).
 * ------------------------------------------------------------------------------------------ */
typedef struct aos2_vis aos2_vis_t;

typedef struct {
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;   /* MinX, MaxX, MinY, MaxY: the window of :285-289 */
    float max_dist, min_dist;           /* :293 */
    int32_t feature_threshold;
    float T_sw[16], T_bc[16];           /* row-major */
} aos2_vis_camera_t;
#define AOS2_VIS_CAMERA_MAP 0     /* camera(map_data, int) :5-70:  window 930 / 10 / 520 / 20, distances 6 / 0.5 */
#define AOS2_VIS_CAMERA_PLAIN 1   /* camera() :105-132:            window 950 / 10 / 530 / 10, distances 6 / 0.1, threshold 20 */
/* the constants of one of the reference's constructors (fx .. cy, T_sw and T_bc are the same in both); feature_threshold = 20
 * (camera(map_data, int) takes it from its caller).  They are inputs of the handle, not built in. */
int aos2_vis_camera_default(int which, aos2_vis_camera_t *cam);

/* a handle starts with the AOS2_VIS_CAMERA_MAP constants and an empty map */
int aos2_vis_create(int device, aos2_vis_t **out);
void aos2_vis_destroy(aos2_vis_t *h);
/* AOS2_ERR_ARG if a constant is not finite */
int aos2_vis_set_camera(aos2_vis_t *h, const aos2_vis_camera_t *cam);
/* The planner's map (plan_slam::UpdateMap src/plan.cc:129-139 -> camera(map_data, int) :23-44, which narrows map_data's doubles to
 * float: the caller does the same): xyz [n][3], upper / lower [n] (the viewing-direction bounds), max_range / min_range [n],
 * found_ratio [n].  n == 0 is legal.  The map replaces the one before and stays in HBM until the next call.  Needs no device:
 * the copy goes up with the next count. */
int aos2_vis_set_map(aos2_vis_t *h, int n, const float *xyz, const float *upper, const float *lower, const float *max_range,
                     const float *min_range, const float *found_ratio);
int aos2_vis_map_size(const aos2_vis_t *h);
/* points a workgroup of the gate kernel takes, and states of its tile: the sizes at which the kernel changes block (for tests) */
void aos2_vis_gate_tile(int *points, int *states);

/* countVisible(float x_w, float y_w, float theta_rad_w) :135-167 for ns states [ns][3] = x, y, theta: count [ns] =
 * int(round(num_visible)).  Optional (NULL: not wanted): sum [ns] = num_visible itself, the ratios of the passing points added in
 * point order; mask [ns][ceil(n / 64)]: bit i % 64 of word i / 64 says that point i passed isInFrustum.  ns == 0 is AOS2_OK. */
int aos2_vis_count(aos2_vis_t *h, int ns, const float *states, int32_t *count, float *sum, uint64_t *mask);
/* countVisible(cv::Mat Twb) :170-198: T_wb [ns][16] row-major float */
int aos2_vis_count_poses(aos2_vis_t *h, int ns, const float *T_wb, int32_t *count, float *sum, uint64_t *mask);
/* StateValidChecker::MotionCostCamera (src/StateValidChecker.cc:531-541) for nm motions in one call: motion m is the states
 * offsets[m] .. offsets[m + 1] - 1 of states [offsets[nm]][3]; cost [nm] = the terms c < thres ? 1./1e-4 : 1./c of its states
 * 1 .. size - 2, added in index order (sizes 1 and 2 give 0).  A motion of size 0 is AOS2_ERR_ARG (the reference's Q.size()-1
 * underflows there), as are offsets that do not start at 0 or descend.  thres < 0: the camera's feature_threshold. */
int aos2_vis_motion_costs(aos2_vis_t *h, int nm, const int32_t *offsets, const float *states, int thres, double *cost);
/* plan_slam::AdvanceStepCamera (src/plan.cc:141-151) over IsStateVisiblilty (src/camera.cc:242-250): *index = the last index of
 * the leading run of states with count > thres, -1 if the first state fails (or ns == 0).  thres == -1: feature_threshold. */
int aos2_vis_advance(aos2_vis_t *h, int ns, const float *states, int thres, int32_t *index);
float aos2_vis_last_device_ms(const aos2_vis_t *h);   /* device time of the last call's kernels (HIP events) */

/* ------------------------------------------------------------------------------------------
 * StateValidChecker (planner motion checks)  (include/StateValidChecker.h:47-150, src/StateValidChecker.cc, src/collisions.cc)
 * What RRT* asks for every neighbour of a new node (src/myRRTstar.cc:302-464): the two-wheel shortest path between two states
 * (GetShortestPath :313-367), its states in steps of dt (myprop :296-311), isValid of each (:97-119 = check_collisions
 * src/collisions.cc:70-94, then camera::IsStateVisiblilty) and the two motion costs (:522-578).  The reference does this for one
 * pair of states per call, serially; here a call takes a batch of (q1, q2) pairs.  All of it is double arithmetic with sin, cos and
 * atan2 as fixed operation sequences (csrc/motion_tw.h), so the device, the host taps and the tests' restatement agree bit for
 * bit.
 * A state is x, y, theta.  A component that is not finite, or |theta| > 1e4, is AOS2_ERR_ARG (csrc/motion_tw.h says why).
 * ------------------------------------------------------------------------------------------ */
typedef struct aos2_svc aos2_svc_t;

typedef struct {
    double turn_radius, robot_r, dt;       /* TURN_RADIUS 0.25, ROBOT_RADIUS 0.4, DT 0.3  include/StateValidChecker.h:28-30 */
    double min_x, max_x, min_y, max_y;     /* MIN_X -1.15, MAX_X 6.5, MIN_Y -5, MAX_Y 5   include/collisions.h:30-33 */
    double max_dist_heuristic;             /* MAX_DIST_HEURISTIC 2  include/StateValidChecker.h:31 */
    double start[3];                       /* StartState (setStartState :76-80); read only with `heuristic` */
    int32_t heuristic;                     /* heuristicValidityCheck, 0 as every constructor of the reference leaves it */
    int32_t feature_threshold;             /* -1: the feature_threshold of the handle's camera */
} aos2_svc_params_t;
#define AOS2_SVC_MAX_SEGMENT_STATES (1 << 20)   /* states one of a path's three segments may have; more is AOS2_ERR_ARG */

int aos2_svc_params_default(aos2_svc_params_t *p);
/* a handle starts with the default parameters, no obstacles, and a visibility handle with the AOS2_VIS_CAMERA_MAP constants and an
 * empty map */
int aos2_svc_create(int device, aos2_svc_t **out);
void aos2_svc_destroy(aos2_svc_t *h);
/* the camera base of the class: the handle's own visibility handle (it dies with the handle).  Camera and map are set on it with
 * aos2_vis_set_camera / aos2_vis_set_map. */
aos2_vis_t *aos2_svc_vis(aos2_svc_t *h);
/* AOS2_ERR_ARG if a value is not finite, or turn_radius or dt is not positive */
int aos2_svc_set_params(aos2_svc_t *h, const aos2_svc_params_t *p);
/* collisionDetection(ppMatrix FloorMap) src/collisions.cc:23-37: xy [n][2]; obs_r is the class's 0.1 (include/collisions.h:61)
 * unless the caller loaded a file (load_obstacles :39-64 takes the last row's r).  n == 0 is legal and makes check_collisions true
 * for every state (:73).  The obstacles replace the ones before and stay in HBM until the next call.  Needs no device. */
int aos2_svc_set_obstacles(aos2_svc_t *h, int n, const double *xy, double obs_r);
/* obstacles a workgroup of the collision kernel stages at a time, and states of its tile (for tests) */
void aos2_svc_collide_tile(int *obstacles, int *states);

/* StateValidChecker::isValid(Vector) :97-119 for ns states [ns][3] (Planning.cc:190, checkMotion's interpolated states :121-161).
 * valid [ns]; optional: collision_free [ns] = check_collisions(q, robot_r), count [ns] = countVisible of the state narrowed to
 * float, for every state whether or not isValid reaches it. */
int aos2_svc_valid(aos2_svc_t *h, int ns, const double *states, uint8_t *valid, uint8_t *collision_free, int32_t *count);

typedef struct {
    /* per motion, [nm] unless said otherwise; NULL: not wanted */
    uint8_t *path_valid;     /* GetShortestPath(q1, q2).valid :313-367 */
    int32_t *type;           /* the winning candidate in the order of the loops :337-339, (s1, s2, dir) = (-1,-1,-1) is 0, (-1,-1,1) is 1,
                                .. (1,1,1) is 7; -1 without a path */
    double *t;               /* [nm][3] vwt.t; zeros without a path */
    int32_t *m;              /* [nm][3] 1 + ceil(t[i] / dt) :259; zeros without a path */
    int32_t *n_states;       /* Q.size() of reconstructMotionTW :273-294 (1 without a path: MotionCost's Q = {q1} :561-562) */
    uint8_t *valid;          /* checkMotionTW :244-271 */
    int32_t *first_invalid;  /* the index into Q of the state at which checkMotionTW returns false, -1 if none does */
    double *cost_length;     /* MotionCost(s1, s2, 1) :543-578 */
    double *cost_camera;     /* MotionCost(s1, s2, 2) */
    /* reconstructMotionTW of every motion: motion k is the states offsets[k] .. offsets[k + 1] - 1 */
    int32_t *offsets;        /* [nm + 1] */
    double *states;          /* [states_capacity][3] */
    int64_t states_capacity; /* in: rows `states` holds */
    int64_t states_needed;   /* out: the rows all motions have together, also when the call fails with AOS2_ERR_CAPACITY */
} aos2_svc_motions_out_t;
/* q1, q2 [nm][3].  With `states` set and states_capacity below the total: AOS2_ERR_CAPACITY, states_needed says how many rows are
 * needed and no output is written.  nm == 0 is AOS2_OK. */
int aos2_svc_motions(aos2_svc_t *h, int nm, const double *q1, const double *q2, aos2_svc_motions_out_t *out);
float aos2_svc_last_device_ms(const aos2_svc_t *h);   /* device time of the last call (HIP events; aos2_svc_motions: its one host wait included) */

/* ------------------------------------------------------------------------------------------
 * ORBmatcher  (include/ORBmatcher.h:37-102, src/ORBmatcher.cc)
 * The C++ shim snapshots the Frame / KeyFrame / MapPoint fields each method reads into the SoA
 * views below and maps the returned indices back to MapPoint*.
 * ------------------------------------------------------------------------------------------ */
#define AOS2_TH_HIGH 100     /* ORBmatcher::TH_HIGH  src/ORBmatcher.cc:37 */
#define AOS2_TH_LOW 50       /* ORBmatcher::TH_LOW   :38 */
#define AOS2_HISTO_LENGTH 30 /* ORBmatcher::HISTO_LENGTH :39 */
#define AOS2_GRID_COLS 64    /* FRAME_GRID_COLS include/Frame.h:38 */
#define AOS2_GRID_ROWS 48    /* FRAME_GRID_ROWS include/Frame.h:37 */

typedef struct aos2_matcher aos2_matcher_t;

/* ORBmatcher::ORBmatcher(float nnratio=0.6, bool checkOri=true)  src/ORBmatcher.cc:41-43 */
int aos2_matcher_create(float nnratio, int check_orientation, int device, aos2_matcher_t **out);
void aos2_matcher_destroy(aos2_matcher_t *m);

/* device time (ms, HIP events) of the kernels of the last search_* call on this handle */
float aos2_matcher_last_device_ms(const aos2_matcher_t *m);

/* static int ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&)  :1647-1663.
 * Host scalar helper (pure); the device kernels use xor + popcount of the same 256 bits. */
int aos2_descriptor_distance(const uint8_t *a, const uint8_t *b);

/* Brute-force Hamming: for every query descriptor the best and second best train descriptor.
 * q[nq][32], t[nt][32] host memory.  best_idx/best_dist/second_dist: nq entries.
 * Ties: lowest train index wins (strict '<' update order of the reference loops). */
int aos2_matcher_hamming_best2(aos2_matcher_t *m, const uint8_t *q, int nq, const uint8_t *t,
                               int nt, int32_t *best_idx, int32_t *best_dist,
                               int32_t *second_dist);
/* device-resident variant + kernel timing (ms, HIP events) for the roofline/throughput report */
int aos2_matcher_hamming_best2_device(aos2_matcher_t *m, const uint8_t *d_q, int nq,
                                      const uint8_t *d_t, int nt, int32_t *d_best_idx,
                                      int32_t *d_best_dist, int32_t *d_second_dist, int iters,
                                      float *avg_ms);

typedef struct {
    int32_t n_kf, n_f;
    const uint8_t *desc_kf;    /* pKF->mDescriptors, n_kf x 32 */
    const uint8_t *desc_f;     /* F.mDescriptors, n_f x 32 */
    const uint8_t *kf_has_mp;  /* n_kf: vpMapPointsKF[i] != NULL && !isBad() (:194-198) */
    const float *angle_kf;     /* pKF->mvKeysUn[i].angle */
    const float *angle_f;      /* F.mvKeys[j].angle */
    /* DBoW2::FeatureVector (std::map<NodeId, vector<unsigned>>) flattened to CSR with node ids
     * ascending: Thirdparty/DBoW2/DBoW2/FeatureVector.h:21-22 */
    int32_t n_nodes_kf, n_nodes_f;
    const int32_t *node_id_kf, *node_off_kf, *node_idx_kf;
    const int32_t *node_id_f, *node_off_f, *node_idx_f;
} aos2_bow_pair_t;

/* int ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)  src/ORBmatcher.cc:159-288.
 * `n_pairs` independent (KF, F) pairs are matched in one launch (one workgroup per pair).
 * match_f[p] (n_f entries): index of the KF feature whose MapPoint is assigned to frame feature j,
 * or -1 (NULL).  nmatches[p] = return value. */
int aos2_matcher_search_by_bow(aos2_matcher_t *m, const aos2_bow_pair_t *pairs, int n_pairs,
                               int32_t *const *match_f, int32_t *nmatches);

/* The same search on frames whose descriptors and keys already live in HBM (a device-resident Frames batch, the
 * extractor's device outputs): desc_kf / desc_f / angle_kf / angle_f of the pairs are DEVICE arrays and are used in place
 * (32 KB + 4 KB per frame that do not cross PCIe); kf_has_mp, the FeatureVector CSRs (the host merge-joins them, :181-258)
 * and the results are host arrays, a few KB per pair.  The caller has completed (or ordered this handle's work behind) the
 * producers of the device arrays. */
int aos2_matcher_search_by_bow_device(aos2_matcher_t *m, const aos2_bow_pair_t *pairs, int n_pairs,
                                      int32_t *const *match_f, int32_t *nmatches);

/* The per-keyframe front part of Tracking::TrackReferenceKeyFrame (src/Tracking.cc:858-866) for `n_frames` (reference
 * keyframe b, frame b) pairs whose members live in HBM as the extractor and aos2_vocabulary_transform_device wrote them:
 * descriptors [n][cap][32], keypoints [n][cap] (mvKeys: the angle is read), counts [n], FeatureVectors fv_node [n][cap],
 * fv_off [n][cap + 1], fv_idx [n][cap], n_fv [n] -- all DEVICE arrays; kf_has_mp [n][cap] is a HOST array (map state:
 * vpMapPointsKF[i] != NULL && !isBad()).  The call copies the FeatureVectors and counts to the host (a few KB per frame),
 * merge-joins them there, and runs aos2_matcher_search_by_bow_device.  match_f: HOST [n][cap], nmatches: HOST [n]. */
typedef struct {
    int32_t n_frames, cap;
    const uint8_t *d_desc_kf;          const aos2_keypoint_t *d_kps_kf;  const int32_t *d_n_kf;
    const uint8_t *d_desc_f;           const aos2_keypoint_t *d_kps_f;   const int32_t *d_n_f;
    const uint8_t *kf_has_mp;
    const int32_t *d_kf_fv_node, *d_kf_fv_off, *d_kf_fv_idx, *d_kf_n_fv;
    const int32_t *d_f_fv_node, *d_f_fv_off, *d_f_fv_idx, *d_f_n_fv;
} aos2_bow_frames_t;
int aos2_matcher_search_by_bow_frames(aos2_matcher_t *m, const aos2_bow_frames_t *q, int32_t *match_f,
                                      int32_t *nmatches);

/* int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12)
 * src/ORBmatcher.cc:522-655 (LoopClosing.cc:? / Tracking relocalisation candidates).
 * has_mp*: GetMapPointMatches()[i] != NULL && !isBad().  match12[p] (n1 entries): index of the KF2
 * feature whose MapPoint becomes vpMatches12[i], or -1 (NULL). */
typedef struct {
    int32_t n1, n2;
    const uint8_t *desc1, *desc2;      /* mDescriptors */
    const uint8_t *has_mp1, *has_mp2;
    const float *angle1, *angle2;      /* mvKeysUn[i].angle */
    int32_t n_nodes1, n_nodes2;        /* mFeatVec as CSR, node ids ascending */
    const int32_t *node_id1, *node_off1, *node_idx1;
    const int32_t *node_id2, *node_off2, *node_idx2;
} aos2_bow_kf_pair_t;
int aos2_matcher_search_by_bow_kf(aos2_matcher_t *m, const aos2_bow_kf_pair_t *pairs, int n_pairs,
                                  int32_t *const *match12, int32_t *nmatches);

/* int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12,
 *         vector<pair<size_t,size_t>> &vMatchedPairs, const bool bOnlyStereo)   src/ORBmatcher.cc:657-823
 * (LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:? calls it once per neighbour keyframe:
 * `n_pairs` (pKF1, pKF2_k) problems go in one launch).  has_mp*: GetMapPoint(i) != NULL.
 * F12: row-major 3x3 (LocalMapping::ComputeF12); ex, ey: the epipole of :664-670.
 * match12[p] (n1 entries) = vMatches12 (KF2 feature index or -1); vMatchedPairs is its non-negative
 * entries in ascending i (:811-820).  nmatches[p] = return value. */
typedef struct {
    int32_t n1, n2;
    const uint8_t *desc1, *desc2;
    const uint8_t *has_mp1, *has_mp2;
    const float *x1, *y1, *angle1, *u_right1;   /* pKF1->mvKeysUn[i].pt / .angle, mvuRight */
    const float *x2, *y2, *angle2, *u_right2;
    const int32_t *octave2;                     /* pKF2->mvKeysUn[i].octave */
    const float *scale_factors2, *level_sigma2_2;  /* pKF2->mvScaleFactors / mvLevelSigma2 */
    int32_t n_levels2;
    float F12[9];
    float ex, ey;
    int32_t n_nodes1, n_nodes2;                 /* mFeatVec as CSR */
    const int32_t *node_id1, *node_off1, *node_idx1;
    const int32_t *node_id2, *node_off2, *node_idx2;
} aos2_triang_pair_t;
int aos2_matcher_search_for_triangulation(aos2_matcher_t *m, const aos2_triang_pair_t *pairs,
                                          int n_pairs, int only_stereo, int32_t *const *match12,
                                          int32_t *nmatches);

/* void MapPoint::ComputeDistinctiveDescriptors()  src/MapPoint.cc:275-340, for a batch of map points:
 * the descriptors observed for point p (rows of the non-bad keyframes, in std::map order, :297-303) are
 * desc[off[p] .. off[p+1]).  best_idx[p] = index inside that list of the descriptor with the least
 * median distance to the others (first one on ties), -1 for an empty list. */
int aos2_compute_distinctive_descriptors(aos2_matcher_t *m, int n_points, const int32_t *off,
                                         const uint8_t *desc, int32_t *best_idx);

typedef struct {
    int32_t n_f;
    const uint8_t *desc_f;      /* F.mDescriptors */
    const float *kp_x, *kp_y;   /* F.mvKeysUn[i].pt */
    const int32_t *kp_octave;   /* F.mvKeysUn[i].octave */
    const float *kp_angle;      /* F.mvKeysUn[i].angle */
    const float *u_right;       /* F.mvuRight */
    const float *scale_factors; /* F.mvScaleFactors */
    int32_t n_levels;
    float min_x, min_y, max_x, max_y; /* F.mnMinX, mnMinY, mnMaxX, mnMaxY */
    float grid_w_inv, grid_h_inv;     /* F.mfGridElementWidthInv / HeightInv */
    /* F.mGrid[64][48] as CSR, cell = ix*48 + iy (src/Frame.cc:259-274) */
    const int32_t *grid_off, *grid_idx;
    /* per feature: 0 = mvpMapPoints[i]==NULL, 1 = map point with Observations()==0,
     * 2 = map point with Observations()>0 (the skip test of :87-89 / :1403-1405) */
    const uint8_t *f_mp_state;
} aos2_frame_view_t;

typedef struct {
    int32_t n_mp;
    const uint8_t *track_in_view; /* pMP->mbTrackInView && !pMP->isBad() (:52-56) */
    const int32_t *pred_level;    /* mnTrackScaleLevel */
    const float *view_cos;        /* mTrackViewCos */
    const float *proj_x, *proj_y, *proj_xr; /* mTrackProjX / Y / XR */
    const uint8_t *desc;          /* pMP->GetDescriptor(), n_mp x 32 */
    const uint8_t *has_obs;       /* pMP->Observations() > 0 */
} aos2_proj_mp_t;

/* int ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, const float th)
 * src/ORBmatcher.cc:45-129.  match_f[n_f]: index into the map point list newly assigned to
 * F.mvpMapPoints[j], or -1 = entry unchanged.  Any number of map points: beyond n_mp x n_f x 8 B = 64 MB the scratch
 * for the candidates is sized from the real window populations (two passes) instead of n_mp x n_f slots.
 * AOS2_ERR_ARG (before anything is uploaded) if the frame view or the point set is inconsistent: non-monotone grid
 * offsets, grid entries or pyramid levels out of range, NULL arrays. */
int aos2_matcher_search_by_projection(aos2_matcher_t *m, const aos2_frame_view_t *f,
                                      const aos2_proj_mp_t *p, float th, int32_t *match_f,
                                      int32_t *nmatches);

/* The same search for `n_problems` independent (frame, local map points) problems in one launch (one
 * greedy-resolve wave per frame, all frames in flight together): replaying or relocalising many frames.
 * match_f[i] has frames[i].n_f entries.  The candidate-entry pool is budgeted at 512 features per search
 * window; AOS2_ERR_CAPACITY if the windows of a batch hold more (then call the per-frame entry point). */
int aos2_matcher_search_by_projection_batch(aos2_matcher_t *m, const aos2_frame_view_t *frames,
                                            const aos2_proj_mp_t *problems, int n_problems, float th,
                                            int32_t *const *match_f, int32_t *nmatches);

typedef struct {
    int32_t n_last;
    const uint8_t *last_valid;  /* LastFrame.mvpMapPoints[i] && !LastFrame.mvbOutlier[i] */
    const float *world_pos;     /* pMP->GetWorldPos(), n_last x 3 float32 */
    const uint8_t *desc;        /* pMP->GetDescriptor(), n_last x 32 */
    const int32_t *last_octave; /* LastFrame.mvKeys[i].octave */
    const float *last_angle;    /* LastFrame.mvKeysUn[i].angle */
    const uint8_t *has_obs;     /* pMP->Observations() > 0 */
    float Tcw[16], Tlw[16];     /* CurrentFrame.mTcw, LastFrame.mTcw: row-major 4x4 float32 */
    float fx, fy, cx, cy, mb, mbf;
} aos2_proj_last_t;

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th,
 * const bool bMono)  src/ORBmatcher.cc:1328-1470.  match_f[n_f]: last-frame feature index whose
 * MapPoint is assigned, -1 = unchanged, -2 = reset to NULL by the rotation-histogram cull. */
int aos2_matcher_search_by_projection_last(aos2_matcher_t *m, const aos2_frame_view_t *cur,
                                           const aos2_proj_last_t *p, float th, int mono,
                                           int32_t *match_f, int32_t *nmatches);

/* Projection family: a set of map points projected into a keyframe / frame (aos2_frame_view_t; for a
 * KeyFrame the view carries mvKeysUn, mvuRight, mDescriptors, mGrid, mnMin/Max*, mvScaleFactors; f_mp_state
 * is used by the two greedy searches only).  Rotations are row-major 3x3.  The few cv::Mat lines that
 * decompose Scw or build sR12 / sR21 / t21 (:299-304, :986-991, :1116-1120) stay in the caller: R, t, Ow
 * (and R2, t2) are inputs, so no OpenCV rounding behaviour is guessed on the device. */
typedef struct {
    int32_t n_pts;
    const uint8_t *valid;            /* the per-point gate of the reference loop head, see each function */
    const float *pos;                /* 3 per point: GetWorldPos() */
    const float *max_dist, *min_dist;   /* MapPoint::mfMaxDistance / mfMinDistance, RAW (include/MapPoint.h:149-150): the range gate applies
                                      * Get{Max,Min}DistanceInvariance()'s 1.2f / 0.8f (src/MapPoint.cc:413-423) on the device and
                                      * MapPoint::PredictScale (:427-459) divides the raw maximum by the distance */
    const float *normal;             /* 3 per point: GetNormal() (unused by SearchBySim3 and the reloc search) */
    const uint8_t *desc;             /* 32 per point: GetDescriptor() */
    const float *q_angle;            /* reloc search only: pKF->mvKeysUn[i].angle */
    float R[9], t[3], Ow[3];         /* Rcw, tcw, camera centre */
    float R2[9], t2[3];              /* SearchBySim3 only: sR21, t21 (KF1 -> KF2) or sR12, t12 */
    float fx, fy, cx, cy, bf;        /* bf: Fuse(pKF, vpMapPoints) only (ur = u - bf*invz, :870) */
    float log_scale_factor;          /* mfLogScaleFactor of the target (MapPoint::PredictScale) */
    const float *inv_level_sigma2;   /* mvInvLevelSigma2 of the target, Fuse(pKF, vpMapPoints) only */
    float th;
} aos2_proj_points_t;

/* The search part of int ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)  :825-975  (sim3 = 0,
 * valid[i] = pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF)) and of Fuse(KeyFrame*, cv::Mat Scw,
 * vpPoints, th, vpReplacePoint)  :977-1100 (sim3 = 1, valid[i] = !isBad() && !spAlreadyFound.count(pMP)).
 * best_idx[i] = the keyframe feature the point fuses with (bestDist <= TH_LOW), -1 otherwise;
 * best_dist[i] its distance; *n_fused = the count.  The Replace / AddObservation / vpReplacePoint
 * bookkeeping of :950-969 / :1079-1093 consumes best_idx on the host (it only reads map state). */
int aos2_matcher_fuse(aos2_matcher_t *m, const aos2_frame_view_t *kf, const aos2_proj_points_t *p,
                      int sim3, int32_t *best_idx, int32_t *best_dist, int32_t *n_fused);

/* int ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*> &vpPoints,
 *         vector<MapPoint*> &vpMatched, int th)  :290-403.  valid[i] = !isBad() && !spAlreadyFound.count;
 * kf->f_mp_state[idx] != 0 <=> vpMatched[idx] != NULL on entry.  match_f[idx] = index of the point
 * written to vpMatched[idx], -1 = unchanged. */
int aos2_matcher_search_by_projection_kf(aos2_matcher_t *m, const aos2_frame_view_t *kf,
                                         const aos2_proj_points_t *p, int32_t *match_f,
                                         int32_t *nmatches);

/* int ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)  :1102-1326.
 * p12: one entry per KF1 feature (valid = pMP && !vbAlreadyMatched1[i] && !isBad(); R, t = R1w, t1w;
 * R2, t2 = sR21, t21), projected into kf2; p21 the converse (R2w, t2w; sR12, t12) into kf1.
 * match12[i1] = KF2 feature index whose map point becomes vpMatches12[i1], -1 = unchanged. */
int aos2_matcher_search_by_sim3(aos2_matcher_t *m, const aos2_frame_view_t *kf1,
                                const aos2_frame_view_t *kf2, const aos2_proj_points_t *p12,
                                const aos2_proj_points_t *p21, int32_t *match12, int32_t *n_found);

/* The RANSAC of Sim3Solver (src/Sim3Solver.cc: SetRansacParameters :114-138, iterate :140-207, ComputeSim3 :226-337, CheckInliers
 * :340-364) for a batch of candidate keyframes of LoopClosing::ComputeSim3 (src/LoopClosing.cc:276-303), between SearchByBoW (:267)
 * and SearchBySim3 (:325).  The random triples are an input, so the hypotheses are independent: every hypothesis of every problem
 * is computed in one pass and the solver's sequential loop (:183-199) is replayed over the inlier counts.  The arithmetic is
 * csrc/sim3.h. */
typedef struct {
    int32_t n;                       /* correspondences that survived the constructor's gates (:62-103): N */
    const float *X3Dc1, *X3Dc2;      /* host [n][3]: mvX3Dc1 / mvX3Dc2 = Rcw*X3Dw + tcw, formed by the caller (:94-98) */
    const float *max_err1, *max_err2;/* host [n]: 9.210 * mvLevelSigma2[octave] as float (:84-88); the class keeps them in a
                                      * vector<size_t> (include/Sim3Solver.h:78-79), host/Sim3Solver.h passes those whole numbers */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;   /* mK1, mK2 */
    int32_t fix_scale;               /* mbFixScale */
    double probability; int32_t min_inliers, max_iterations;   /* SetRansacParameters (:114); max_iterations >= 1 */
    const int32_t *draws;            /* host [max_iterations][3]: draw i of an iteration = RandomInt(0, n-1-i) (:168); not read when
                                      * n < min_inliers */
} aos2_sim3_problem_t;
typedef struct {
    int32_t ransac_max_its;          /* mRansacMaxIts after :125-135 (a quotient that is no int converts as x86 does: INT_MIN, so 1) */
    int32_t first_success;           /* 0-based iteration at which iterate() would return a Sim3, -1 = never */
    int32_t best_iteration, best_inliers;   /* the solver's mBest* state when it stops (at first_success, or after ransac_max_its);
                                             * best_iteration = -1 when nothing ran */
    float T12[16], R12[9], t12[3], s12;     /* mBestT12 / mBestRotation / mBestTranslation / mBestScale (zeros when nothing ran) */
    uint8_t *inliers;                /* host [n], caller-allocated: mvbBestInliers */
    int32_t *counts;                 /* host [max_iterations] or NULL: mnInliersi per iteration that ran, -1 beyond the stop */
} aos2_sim3_result_t;
/* n_problems <= 64; n_problems == 0 is AOS2_OK.  n < min_inliers (:146-150): ransac_max_its as computed, first_success = -1,
 * best_inliers = 0, no inlier flag set, nothing launched for that problem.  The three indices of iteration k follow from draws[k] by
 * the swap-with-back removal of :163-177.  A draw outside [0, n-1-i], n < 0, n < 3 with something to run, max_iterations < 1 or a
 * missing array is AOS2_ERR_ARG, reported before anything runs (no result is written).  A degenerate triple is no error: its model
 * holds NaNs, every comparison of :356 is false and its count is 0, as in the reference.  Hypotheses after first_success are
 * computed by the batch but reported as if they had not run.  Synchronous. */
int aos2_sim3_ransac(aos2_matcher_t *m, const aos2_sim3_problem_t *problems, aos2_sim3_result_t *results, int n_problems);

/* The RANSAC of PnPsolver (src/PnPsolver.cc: SetRansacParameters :121-157, iterate :165-258, Refine :260-305, CheckInliers :308-339,
 * compute_pose :477-525 = EPnP) for a batch of relocalisation candidates of Tracking::Relocalization (src/Tracking.cc:1521-1700),
 * between SearchByBoW (:1557) and PoseOptimization (:1620).  The random minimal sets are an input, so every hypothesis of every
 * problem is independent, and Refine() is a function of the best set alone: all hypotheses, then the Refine() of every iteration
 * that sets a new best, are computed in one pass and the solver's sequential loop (:182-239) is replayed over the inlier counts and
 * those memoised results.  The arithmetic is csrc/pnp.h.
 *
 * SetRansacParameters (:121-157) as a pure host function, no device: the adjusted mRansacMinInliers, mRansacEpsilon, mRansacMaxIts.
 * A quotient (or N*epsilon) that is no int converts as x86 does (INT_MIN, so 1: item 9's rule).  n < 0 or a missing output is
 * AOS2_ERR_ARG. */
int aos2_pnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                               int32_t *ransac_min_inliers, float *ransac_epsilon, int32_t *ransac_max_its);
typedef struct {
    int32_t n;                       /* N: correspondences the constructor kept (:79-101) */
    const float *P3Dw, *P2D, *max_err;   /* host [n][3], [n][2], [n]: mvP3Dw, mvP2D (mvKeysUn[i].pt), mvMaxError = mvSigma2 * th2, a
                                          * float product (:156) */
    float fx, fy, cx, cy;            /* F.fx ...; widened to the class's double fu fv uc vc (:104-107) */
    int32_t min_inliers, min_set;    /* the ADJUSTED mRansacMinInliers (aos2_pnp_ransac_parameters); 4 <= min_set <= 16 */
    int32_t first_iteration, n_iterations;   /* the call replays iterations [first_iteration, n_iterations) of the solver (0-based
                                              * values of mnIterations before its increment, :185) */
    const int32_t *draws;            /* host [n_iterations][min_set]: draw i of an iteration = RandomInt(0, n-1-i) (:193); rows below
                                      * first_iteration are not read */
    int32_t best_inliers_in;         /* the solver's state carried in: mnBestInliers (0 at the start) ... */
    const uint8_t *best_in;          /* ... and mvbBestInliers [n] (NULL when best_inliers_in == 0) */
} aos2_pnp_problem_t;
typedef struct {
    int32_t returned_at;             /* iteration at which iterate() returns a refined pose (:226-236), -1 = ran to n_iterations */
    float Tcw[16];                   /* mRefinedTcw (:294-300) */
    int32_t n_inliers;               /* mnRefinedInliers */
    uint8_t *inliers;                /* host [n], caller-allocated: mvbRefinedInliers (zeros while returned_at < 0) */
    int32_t best_iteration, best_inliers;   /* mnBestInliers where the call stops and the iteration that set it; best_iteration =
                                             * -1: the carried-in best still stands */
    float best_Tcw[16];              /* mBestTcw (:217-223); zeros while best_iteration < 0 (the caller keeps its own) */
    uint8_t *best;                   /* host [n], caller-allocated: mvbBestInliers (best_in while best_iteration < 0) */
    int32_t *counts;                 /* host [n_iterations] or NULL: mnInliersi of the iterations that ran, -1 elsewhere */
} aos2_pnp_result_t;
/* n_problems <= 64; n_problems == 0 is AOS2_OK.  Checked before anything runs, AOS2_ERR_ARG with no result byte written: a draw
 * outside [0, n-1-i], n < 0, n < min_set with something to run, min_set outside [4, 16], a missing array, first_iteration < 0 or
 * > n_iterations, best_inliers_in < 0, best_inliers_in > 0 without best_in.  n < min_inliers (:173-177) or first_iteration ==
 * n_iterations: nothing is launched for that problem, returned_at = -1, counts -1.  A degenerate minimal set is no error: its model
 * holds NaNs, every comparison of :329 is false and its count is 0.  Iterations behind returned_at are computed by the batch but
 * reported as not run.  A result is a function of its problem alone: the same bytes whatever else is in the batch.  A call resumed
 * with first_iteration = returned_at + 1 (or n_iterations), best_inliers_in = best_inliers and best_in = best gives what the
 * uninterrupted loop gives; an iteration with count >= min_inliers that does not beat the carried best runs Refine() on the carried
 * set.  Synchronous. */
int aos2_pnp_ransac(aos2_matcher_t *m, const aos2_pnp_problem_t *problems, aos2_pnp_result_t *results, int n_problems);

/* Initializer::Initialize (src/Initializer.cc:44-121) for a batch of monocular sequences, behind SearchForInitialization of
 * Tracking::MonocularInitialization (src/Tracking.cc:695, :709): Normalize over all keys of both frames, the homography and the
 * fundamental matrix of every minimal set (ComputeH21 / ComputeF21), CheckHomography / CheckFundamental of each over every match,
 * the pick of the best of each, RH = SH / (SH + SF), then ReconstructH (eight hypotheses) or ReconstructF (four) with CheckRT of
 * every hypothesis over every inlier.  The minimal sets are an input (mvSets), so every hypothesis is independent.  The arithmetic
 * is csrc/initializer.h. */
#define AOS2_INIT_OK 0
#define AOS2_INIT_NO_MODEL 1         /* no hypothesis of the chosen model scored above 0: the reference's next cv::Mat product asserts */
typedef struct {
    int32_t n_keys1, n_keys2;        /* mvKeys1.size(), mvKeys2.size() */
    const float *keys1, *keys2;      /* host [n_keys][2]: mvKeysUn[i].pt of the reference and the current frame */
    int32_t n_matches;               /* mvMatches12.size(), >= 8 */
    const int32_t *matches;          /* host [n_matches][2]: (first, second) in mvMatches12 order */
    float sigma;                     /* mSigma (1.0) */
    int32_t iterations;              /* mMaxIterations (200) */
    const int32_t *sets;             /* host [iterations][8]: mvSets, indices into matches */
    float fx, fy, cx, cy;            /* mK */
    float min_parallax;              /* 1.0 (:116, :118) */
    int32_t min_triangulated;        /* 50 */
} aos2_initializer_problem_t;
typedef struct {
    int32_t status;                  /* AOS2_INIT_OK or AOS2_INIT_NO_MODEL (then everything below the scores is zero) */
    int32_t initialized;             /* what Initialize() returns */
    int32_t used_homography;         /* RH > 0.40 */
    float SH, SF;
    float H21[9], F21[9];            /* the winners (zeros without one) */
    int32_t best_iteration_h, best_iteration_f;   /* the iterations that set them, -1 without one */
    uint8_t *inliers_h, *inliers_f;  /* host [n_matches], caller-allocated: vbMatchesInliersH / F */
    float R21[9], t21[3];            /* zeros unless initialized (the reference leaves empty Mats) */
    float *P3D;                      /* host [n_keys1][3], caller-allocated: vP3D; rows that are not written are zero */
    uint8_t *triangulated;           /* host [n_keys1], caller-allocated: vbTriangulated */
    int32_t n_good[8];               /* nGood of CheckRT per hypothesis, in the reference's order */
    float parallax[8];               /* its parallax in degrees */
    int32_t n_hypotheses;            /* 8 (ReconstructH), 4 (ReconstructF), 0: ReconstructH left at d1/d2 < 1.00001, or no model */
} aos2_initializer_result_t;
/* n_problems <= 64; n_problems == 0 is AOS2_OK.  Checked before anything runs, AOS2_ERR_ARG with no result byte written: a NULL,
 * n_matches < 8, a match index outside its frame, a set entry outside [0, n_matches), iterations < 1, sigma <= 0 (or NaN).
 * Degenerate input is no error: a set that repeats a match, collinear points, a static camera give NaN or zero scores that never
 * win the pick; when that leaves the chosen model without a matrix, status = AOS2_INIT_NO_MODEL and initialized = 0.  A result is
 * a function of its problem alone: the same bytes whatever else is in the batch.  Synchronous. */
int aos2_initializer_initialize(aos2_matcher_t *m, const aos2_initializer_problem_t *problems, aos2_initializer_result_t *results,
                                int n_problems);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*>
 *         &sAlreadyFound, const float th, const int ORBdist)  :1472-1599 (relocalisation).
 * Points = pKF->GetMapPointMatches() (valid = pMP && !isBad() && !sAlreadyFound.count(pMP));
 * frame->f_mp_state[i2] != 0 <=> CurrentFrame.mvpMapPoints[i2] != NULL on entry.
 * match_f[i2]: keyframe feature index whose map point is assigned, -1 unchanged, -2 reset to NULL by the
 * rotation check. */
int aos2_matcher_search_by_projection_reloc(aos2_matcher_t *m, const aos2_frame_view_t *frame,
                                            const aos2_proj_points_t *p, int orb_dist,
                                            int32_t *match_f, int32_t *nmatches);

/* bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit)  src/Frame.cc:298-354, for all the local map
 * points of Tracking::SearchLocalPoints in one call.  p: pos / max_dist / min_dist / normal per point (valid,
 * desc, q_angle unused), R, t, Ow = mRcw, mtcw, mOw, bf = mbf; bounds = mnMinX.. (closed, :319-322).
 * Outputs are the members the search reads: mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR,
 * mnTrackScaleLevel, mTrackViewCos -- i.e. the arrays of aos2_proj_mp_t. */
int aos2_frame_is_in_frustum(aos2_matcher_t *m, const aos2_proj_points_t *p, float min_x, float max_x,
                             float min_y, float max_y, int n_levels, float viewing_cos_limit,
                             uint8_t *track_in_view, float *proj_x, float *proj_y, float *proj_xr,
                             int32_t *pred_level, float *view_cos);

/* void Frame::AssignFeaturesToGrid()  src/Frame.cc:259-274 (+ PosInGrid :411-424): mGrid[64][48] as CSR,
 * cell = ix * 48 + iy, features of a cell in ascending index (= push_back order) -- the grid_off / grid_idx
 * arrays of aos2_frame_view_t.  kp_x / kp_y = mvKeysUn[i].pt.  *n_in_grid = features that fall inside the grid. */
int aos2_frame_assign_features_to_grid(aos2_matcher_t *m, int n, const float *kp_x, const float *kp_y,
                                       float min_x, float min_y, float grid_w_inv, float grid_h_inv,
                                       int32_t *grid_off, int32_t *grid_idx, int32_t *n_in_grid);

/* void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth)  src/Frame.cc:672-693 (the RGB-D configs, e.g.
 * TUM).  kp_x / kp_y = mvKeys[i].pt (distorted, index the depth image by truncation), kpun_x = mvKeysUn[i].pt.x,
 * depth_img: CV_32F, `stride` floats per row.  Outputs mvuRight / mvDepth (-1 where the depth is not positive). */
int aos2_frame_stereo_from_rgbd(aos2_matcher_t *m, int n, const float *kp_x, const float *kp_y,
                                const float *kpun_x, const float *depth_img, int w, int h, int stride,
                                float mbf, float *u_right, float *depth);

/* int ORBmatcher::SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched,
 *         vector<int> &vnMatches12, int windowSize=10)  src/ORBmatcher.cc:405-520 (monocular bootstrap,
 * Tracking::MonocularInitialization).  f2 = view of F2 (grid, mvKeysUn, descriptors); F1 enters through
 * desc1 / octave1 / angle1 (mvKeysUn[i].octave / .angle) and prev_xy = vbPrevMatched (2 floats per F1
 * feature).  match12[n1] = vnMatches12.  The update of :512-515 (vbPrevMatched[i1] = F2 keypoint of the
 * match) is one line in the caller.  n1 < 65535, f2->n_f <= 15000. */
int aos2_matcher_search_for_initialization(aos2_matcher_t *m, const aos2_frame_view_t *f2, int n1,
                                           const uint8_t *desc1, const int32_t *octave1,
                                           const float *angle1, const float *prev_xy,
                                           int window_size, int32_t *match12, int32_t *nmatches);



/* ------------------------------------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment  (include/Optimizer.h:45, src/Optimizer.cc:454-779)
 * The C++ shim gathers the local window from the KeyFrame/MapPoint pointer graph (:457-505)
 * and emits vertices/edges in the reference's order; this call runs :507-744 (g2o graph,
 * 5 + 10 Levenberg-Marquardt iterations with the outlier pass in between) on the device and
 * returns poses/points in the float32 form the reference writes back (:763-778).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_poses;   /* local keyframes first or in any order; fixed flag decides */
    int32_t n_points;
    int32_t n_edges;
    const float *pose_Tcw;      /* n_poses x 16: KeyFrame::GetPose() row-major float32 4x4 */
    const uint8_t *pose_fixed;  /* n_poses: fixed camera, or mnId==0 (:530,:543) */
    const int64_t *pose_id;     /* KeyFrame::mnId (Hessian ordering) */
    const float *point_xyz;     /* n_points x 3: MapPoint::GetWorldPos() float32 */
    const int64_t *point_id;    /* MapPoint::mnId */
    const int32_t *edge_pose;   /* n_edges: index into poses */
    const int32_t *edge_point;  /* n_edges: index into points */
    const float *edge_obs;      /* n_edges x 3: kpUn.pt.x, kpUn.pt.y, mvuRight (ignored for mono) */
    const uint8_t *edge_stereo; /* n_edges: mvuRight >= 0 (:595) */
    const float *edge_inv_sigma2; /* n_edges: pKFi->mvInvLevelSigma2[kpUn.octave] */
    float fx, fy, cx, cy, bf;   /* pKFi->fx ... pKFi->mbf (float members of KeyFrame) */
    const volatile uint8_t *stop_flag; /* bool* pbStopFlag, may be NULL; polled between iterations */
    int32_t iters_first, iters_second; /* 5 and 10 (:661,:708) */
} aos2_lba_problem_t;

typedef struct {
    float *pose_Tcw;         /* n_poses x 16 out: Converter::toCvMat(SE3Quat) (:767) */
    float *point_xyz;        /* n_points x 3 out (:776) */
    uint8_t *edge_outlier;   /* n_edges out: observation to erase (:712-744) */
    double *edge_chi2;       /* n_edges out (may be NULL): e->chi2() at the end */
    int32_t iters_done_first, iters_done_second;  /* iterations SparseOptimizer::optimize() ran (its return value) */
    double final_chi2;       /* robust chi2 of the active edges after the last accepted step */
    double final_lambda;
    float ms_device;         /* device time of the whole call (HIP events; all windows of a batch) */
    int32_t status;          /* AOS2_OK or AOS2_ERR_STOPPED (flag set on entry: outputs equal inputs) */
    int32_t trials_first, trials_second;  /* Levenberg-Marquardt trial steps (solves) of the two optimisations */
    int32_t polls;           /* evaluations of pbStopFlag (SparseOptimizer::terminate()), the entry check included */
    int32_t stop_poll;       /* the evaluation that first saw the flag set, 0 = never */
} aos2_lba_result_t;

typedef struct aos2_lba aos2_lba_t;
int aos2_lba_create(int device, aos2_lba_t **out);
void aos2_lba_destroy(aos2_lba_t *s);
/* void Optimizer::LocalBundleAdjustment(KeyFrame*, bool* pbStopFlag, Map*)  numerical part.
 * Returns AOS2_OK, AOS2_ERR_STOPPED if *stop_flag was set on entry (early return, :656-658;
 * outputs then equal inputs), or an error.
 * The whole procedure (both optimisations, the outlier pass, the inlier check) runs on the device without a host
 * round trip per Levenberg-Marquardt trial; *stop_flag is forwarded to the device while the call waits and is
 * evaluated exactly where g2o evaluates terminate() (optimization_algorithm_levenberg.cpp:149,
 * sparse_optimizer.cpp:372) and where Optimizer.cc:663-666 reads it.  Up to 154 free keyframes: the reduced camera
 * system is factorised in registers up to 40 of them, in device memory beyond, where the panel of the 155th would no longer fit a
 * compute unit's LDS (AOS2_ERR_ARG, before anything runs). */
int aos2_lba_solve(aos2_lba_t *s, const aos2_lba_problem_t *p, aos2_lba_result_t *r);
/* `n_problems` independent windows (several maps, or an offline pass over many windows; SURVEY.md section 8(e):
 * LocalBA = replicas only) in one call: every kernel covers all windows, so their latency-bound Levenberg-Marquardt
 * chains overlap on the device.  results[i].status carries the per-window AOS2_OK / AOS2_ERR_STOPPED; the return
 * value is AOS2_OK unless an argument or HIP error occurred.
 * A handle serves one call at a time (concurrent solves: one handle per calling thread); it keeps its device arena, the
 * host-side structure buffers and the worker threads of the per-window host work between calls. */
int aos2_lba_solve_batch(aos2_lba_t *s, const aos2_lba_problem_t *problems, aos2_lba_result_t *results,
                         int n_problems);
/* Worker threads of a batch's per-window host work (index structures, staging); 0 = default: AOS2_LBA_HOST_THREADS, else
 * min(32, host cores / ranks of the node (LOCAL_WORLD_SIZE or WORLD_SIZE)), never more than windows in the call.  No reference
 * equivalent (g2o builds its structure on the calling thread, sparse_optimizer.cpp:354-372). */
int aos2_lba_set_host_threads(aos2_lba_t *s, int n);
/* Window groups of a batch: 2 = the windows are dealt to two groups whose programs run on streams of their own, half a trial apart,
 * so that one group's reduced systems (one workgroup per window) are factorised while the other's landmark kernels fill the device --
 * the faster form for a batch that has the device to itself (64 mixed windows 5.7 -> 5.2 ms); 1 = one program for all windows -- the
 * faster form when other work shares the device (two handles solving side by side beside the tracking kernels: 61 k against 54 k
 * frames/s of bench.py's composite); 0 = default: 2 for calls of >= 16 windows.  Results do not depend on it.  No reference equivalent. */
int aos2_lba_set_window_groups(aos2_lba_t *s, int n);
/* The device program of the last solve of this handle: `trial_slots` = Levenberg-Marquardt trials enqueued in all (the first round
 * holds as many as there are iterations, for every window of the call; a window whose steps were not all accepted is not finished
 * then and gets a continuation round, sized for what it still needs, with the other unfinished windows only), `host_rounds` = times
 * the host waited for the device (1 = no continuation).  aos2_lba_last_window_slots: the trial slots summed over the windows each
 * round covered -- divided by the trials the windows needed, the lock-step cost of the batch (1.0 = no launch covered a window that
 * had nothing left to do). */
int aos2_lba_last_program(const aos2_lba_t *s, int32_t *trial_slots, int32_t *host_rounds);
int aos2_lba_last_window_slots(const aos2_lba_t *s, int64_t *window_slots);
/* Measurement hook (no device, no reference equivalent): the HOST part of aos2_lba_solve_batch for `n_problems` windows -- the
 * per-window index structures and the staging copies -- on `threads` worker threads; wall milliseconds of the two phases. */
int aos2_lba_debug_host_phase(const aos2_lba_problem_t *problems, int n_problems, int threads, double *build_ms,
                              double *stage_ms);
/* Test hook (no reference equivalent): the stop flag counts as set from its `poll`-th evaluation on (1 = the entry
 * check), as if another thread had set it at that moment; 0 switches the hook off.  Used with
 * aos2_lba_result_t.stop_poll to reproduce an asynchronous abort deterministically. */
int aos2_lba_debug_stop_at_poll(aos2_lba_t *s, int poll);

/* ------------------------------------------------------------------------------------------
 * Optimizer::BundleAdjustment / GlobalBundleAdjustemnt  (include/Optimizer.h:40-44, src/Optimizer.cc:41-237): the whole map,
 * called by LoopClosing::RunGlobalBundleAdjustment (10 iterations, not robust) and Tracking::CreateInitialMapMonocular
 * (20 iterations, robust).  Exactly initializeOptimization(); optimize(iterations): one Levenberg-Marquardt run, no outlier
 * pass.  The reduced camera system is block-sparse (6x6 blocks: pairs of free keyframes that share a map point) and is
 * factorised in device memory in ascending keyframe order, so the number of keyframes is bounded by memory alone.
 * The arithmetic is csrc/global_ba.h.
 * ------------------------------------------------------------------------------------------ */
#define AOS2_ERR_GBA_MEMORY (-7)   /* the map or the factor of its reduced camera system does not fit the memory a call may take, see aos2_last_error() */
typedef struct {
    int32_t iterations;          /* nIterations (>= 1) */
    int32_t robust;              /* bRobust: Huber kernels on the edges */
    float huber_mono, huber_stereo;   /* thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815) as float (:85-86); LocalBA's are sqrt(5.991), sqrt(7.815) */
} aos2_gba_options_t;
typedef struct {
    float *pose_Tcw;             /* n_poses x 16 out: Converter::toCvMat(SE3Quat) of every vertex, the fixed ones included (:199-211) */
    float *point_xyz;            /* n_points x 3 out (:223-234) */
    uint8_t *point_included;     /* n_points out: 0 = the point has no edge (removeVertex, :175-179): point_xyz equals the input bit for bit */
    int32_t iterations, trials;  /* what optimize() returned; Levenberg-Marquardt trial steps (solves) */
    double chi2_initial, chi2_final;   /* activeRobustChi2 of the first linearisation / after the last accepted step */
    double final_lambda;
    int32_t polls, stop_poll;    /* evaluations of pbStopFlag (SparseOptimizer::terminate()); the one that first saw it set, 0 = never */
    int32_t h_blocks, l_blocks;  /* 6x6 blocks below the diagonal of the reduced system / of its factor (the fill of ascending order) */
    float ms_device;             /* device time of the call (HIP events: upload done to last kernel done) */
    int32_t status;              /* AOS2_OK */
} aos2_gba_result_t;
/* One map per call, on the problem description of LocalBundleAdjustment (iters_first / iters_second are ignored): hessian order =
 * free keyframes with an edge by ascending pose_id, then points with an edge by ascending point_id; edges in array order (the
 * caller emits a point's observations by ascending KeyFrame::mnId).  The stop flag is not read on entry: its first evaluation is
 * the head of optimize()'s loop, the later ones the trial loop's and the loop head's again, as in g2o.  A set flag ends the call
 * with the estimates of the last accepted step (AOS2_OK, stop_poll set); aos2_lba_debug_stop_at_poll applies.  n_edges == 0:
 * nothing is optimised (iterations = 0), the poses go through the two conversions.
 * AOS2_ERR_ARG, before anything runs and with no result byte written: iterations < 1, a delta <= 0, a NULL array with a non-zero
 * count, an edge index out of range.  AOS2_ERR_GBA_MEMORY, before anything is enqueued: the call's arena would pass 2 GiB.
 * A zero or NaN pivot is a failed trial (LinearSolverEigen's failure).  Results are a function of the problem alone: bit-identical
 * from call to call (no floating-point atomics; every sum is taken in a fixed order from host-built lists). */
int aos2_global_bundle_adjustment(aos2_lba_t *s, const aos2_lba_problem_t *p, const aos2_gba_options_t *o, aos2_gba_result_t *r);

/* ------------------------------------------------------------------------------------------
 * Optimizer::PoseOptimization  (include/Optimizer.h:46, src/Optimizer.cc:239-452) -- SURVEY §8(f)
 * rank 1, called 1-3 times per frame right after each matcher call (Tracking.cc:870,994,1039).
 * One workgroup per frame runs the whole procedure on the device (4 rounds of up to 10
 * Levenberg-Marquardt iterations on the 6x6 system, outlier reclassification in between);
 * `n_problems` independent frames are solved in one launch.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;                  /* features with a map point (nInitialCorrespondences) */
    const float *Xw;            /* n x 3: pMP->GetWorldPos() */
    const float *obs;           /* n x 3: mvKeysUn[i].pt.x, .pt.y, mvuRight[i] */
    const uint8_t *stereo;      /* n: mvuRight[i] >= 0 */
    const float *inv_sigma2;    /* n: mvInvLevelSigma2[octave] */
    float fx, fy, cx, cy, bf;   /* pFrame->fx .. pFrame->mbf */
    float Tcw[16];              /* pFrame->mTcw, row-major float32 4x4 */
} aos2_pose_problem_t;

typedef struct {
    float Tcw[16];              /* out: pose written by pFrame->SetPose (:446) */
    uint8_t *outlier;           /* out, n entries, caller-allocated: pFrame->mvbOutlier of the features */
    int32_t n_bad;              /* pFrame->nBadPoseOpt */
    int32_t n_inliers;          /* return value: nInitialCorrespondences - nBad (0 if n < 3) */
} aos2_pose_result_t;

/* int Optimizer::PoseOptimization(Frame *pFrame) for a batch of frames; `s` provides device + stream */
int aos2_pose_optimization(aos2_lba_t *s, const aos2_pose_problem_t *problems, aos2_pose_result_t *results,
                           int n_problems);
/* device time (ms, HIP events) of the kernel of the last aos2_pose_optimization call */
float aos2_pose_optimization_last_device_ms(const aos2_lba_t *s);

/* int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
 * const bool bFixScale)  src/Optimizer.cc:1047-1242, for a batch of loop candidates of LoopClosing::ComputeSim3 (:355, between
 * SearchBySim3 and SearchByProjection): both optimisations and the outlier pass of every problem in ONE launch, one workgroup per
 * problem.  The arithmetic is csrc/sim3_opt.h (g2o's central-difference Jacobians kept). */
typedef struct {
    int32_t n;                          /* correspondences that passed :1100-1137, in order of i */
    const float *X1c, *X2c;             /* host [n][3]: P3D1c, P3D2c as the caller forms them (:1119, :1127) */
    const float *obs1, *obs2;           /* host [n][2]: kpUn1.pt, kpUn2.pt */
    const float *inv_sigma2_1, *inv_sigma2_2;   /* host [n] */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    double q12[4], t12[3], s12;         /* g2oS12 in: quaternion (x, y, z, w), translation, scale */
    float th2; int32_t fix_scale;
} aos2_sim3_opt_problem_t;
typedef struct {
    double q12[4], t12[3], s12;         /* g2oS12 out; the input, bit for bit, when the call returns through :1212 */
    uint8_t *outlier;                   /* host [n], caller-allocated: 1 = vpMatches1[idx] set to NULL (:1197 or :1231) */
    int32_t n_bad, n_inliers;           /* nBad of the first pass; the return value */
    int32_t iterations[2], trials[2];   /* diagnostics only: LM iterations / trials of the two optimize() calls.  At convergence the
                                         * sign of rho is rounding noise, so these are NOT reproducible across implementations */
} aos2_sim3_opt_result_t;
/* n_problems <= 64; n_problems == 0 is AOS2_OK.  n == 0: nothing runs, n_inliers = n_bad = 0, S12 out = S12 in.  1 <= n < 10: the
 * first optimisation and its outlier pass run as in the reference and the call returns through :1212 (n_inliers = 0, S12 out = S12
 * in, the flags of the first pass set).  A NULL array with n > 0, n < 0 or th2 <= 0 is AOS2_ERR_ARG, reported before anything runs
 * (no result is written).  Synchronous on the handle's stream.  Results are a function of the problem alone: bit-identical from
 * call to call and whatever else is in the batch. */
int aos2_optimize_sim3(aos2_lba_t *s, const aos2_sim3_opt_problem_t *p, aos2_sim3_opt_result_t *r, int n_problems);
/* device time (ms, HIP events) of the kernel of the last aos2_optimize_sim3 call */
float aos2_optimize_sim3_last_device_ms(const aos2_lba_t *s);

/* void Optimizer::OptimizeEssentialGraph(Map*, KeyFrame *pLoopKF, KeyFrame *pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
 * bFixScale)  src/Optimizer.cc:782-1045, the pose graph of LoopClosing::CorrectLoop (:569): 20 Levenberg-Marquardt iterations over
 * the Sim3 of every keyframe with a block-sparse LDL^T of H + lambda I in device memory (7x7 blocks, eliminated in ascending vertex
 * order, no pivoting), then the SE3 poses (:992-1011) and the corrected map points (:1013-1044).  The caller gathers :798-984: the
 * vertices, the edges in insertion order and their measurements.  The arithmetic is csrc/essential_graph.h (g2o's central-difference
 * Jacobians kept). */
#define AOS2_EG_OK 0
#define AOS2_EG_NO_STEP 1         /* no trial of the first iteration was accepted: the poses are the input's */
#define AOS2_ERR_EG_MEMORY (-6)   /* the factor of a graph (its fill) does not fit the memory a call may take, see aos2_last_error() */
typedef struct {
    int32_t n_vertices;          /* the not-bad keyframes, ascending mnId: index = g2o's hessian order */
    const double *Scw;           /* [n_vertices][8]: q(x,y,z,w), t, s = vScw (:819-833) */
    int32_t fixed;               /* index of pLoopKF */
    int32_t n_edges;             /* in insertion order of :853-984 */
    const int32_t *v0, *v1;      /* vertex 0 (nIDi), vertex 1 (nIDj / parent / loop edge / covisible) */
    const double *Sji;           /* [n_edges][8]: the measurement, formed by the caller */
    int32_t fix_scale, iterations;   /* bFixScale; 20 */
    int32_t n_points;            /* map points that are not bad */
    const float *Xw;             /* [n_points][3] GetWorldPos() */
    const int32_t *ref;          /* [n_points] vertex index of nIDr (:1021-1030) */
} aos2_essential_graph_problem_t;
typedef struct {
    double *Scw;                 /* [n_vertices][8] corrected Siw (the fixed one bit-identical to its input) */
    float  *Tiw;                 /* [n_vertices][16] :1002-1008: R(q), t * (1./s) */
    float  *Xw;                  /* [n_points][3] :1038-1040 */
    double chi2_initial, chi2_final;
    int32_t iterations, trials, rejected;   /* diagnostics, as in aos2_sim3_opt_result_t */
    int32_t l_blocks;            /* 7x7 blocks of L below the diagonal: the fill the ordering produced */
    int32_t status;              /* AOS2_EG_OK / AOS2_EG_NO_STEP (no trial of the first iteration was accepted) */
} aos2_essential_graph_result_t;
/* n_problems <= 16; 0 is AOS2_OK.  n_vertices <= 8192.  AOS2_ERR_ARG, before a device is looked for and with no result byte written:
 * a NULL array with a non-zero count, a negative count, n_vertices < 1, fixed / v0 / v1 / ref out of range, v0 == v1, iterations < 1.
 * AOS2_ERR_EG_MEMORY, before anything is enqueued: the memory of L is sized by the symbolic phase and the call's arena would pass
 * 2 GiB.  n_edges == 0 or n_vertices == 1: no LM runs (chi2 = 0, no iterations), poses and points go through the recovery arithmetic
 * with Scw out = Scw in.  Results are a function of the problem alone: bit-identical from call to call and whatever else is in the
 * batch (no floating-point atomics: every block of H, and b, is summed from a host-built list of its edges in edge order). */
int   aos2_optimize_essential_graph(aos2_lba_t *s, const aos2_essential_graph_problem_t *p,
                                    aos2_essential_graph_result_t *r, int n_problems);
/* device time (ms, HIP events: first upload done to last kernel done) of the last aos2_optimize_essential_graph call */
float aos2_optimize_essential_graph_last_device_ms(const aos2_lba_t *s);

/* ------------------------------------------------------------------------------------------
 * Device-resident frame batches: the per-frame chain of Tracking::Track (src/Tracking.cc:862-870, 963-1027, 1302-1352)
 *   ORBextractor::operator() -> Frame::Frame -> SearchByProjection(Current, Last) -> PoseOptimization
 *   -> SearchLocalPoints (isInFrustum + SearchByProjection(F, vpMapPoints)) -> PoseOptimization
 * with the Frame members and the MapPoint table kept in HBM between the calls, so that no
 * keypoint, descriptor, match or pose crosses PCIe inside the chain (the list SearchLocalPoints searches included:
 * aos2_frames_update_local_map, "Tracking::UpdateLocalMap" below, forms it on the device).  A batch is B independent Frames (replaying
 * or relocalising many frames, several cameras, or B (LastFrame, CurrentFrame) pairs); every call is enqueued on the
 * batch's stream and returns without waiting; aos2_frames_wait() waits and reports errors.
 * ------------------------------------------------------------------------------------------ */
typedef struct aos2_frames aos2_frames_t;

/* the members of MapPoint the chain reads (include/MapPoint.h), as a table in device memory; Frames refer to its rows */
typedef struct {
    int32_t n;
    const float *pos;        /* n x 3  GetWorldPos() */
    const uint8_t *desc;     /* n x 32 GetDescriptor() */
    const uint8_t *has_obs;  /* n      Observations() > 0 */
    const float *normal;     /* n x 3  GetNormal()                       (SearchLocalPoints only) */
    const float *min_dist;   /* n      mfMinDistance, raw (gate: 0.8f * it)  (SearchLocalPoints only) */
    const float *max_dist;   /* n      mfMaxDistance, raw (gate: 1.2f * it; PredictScale: it / dist)  (SearchLocalPoints only) */
} aos2_map_points_dev_t;

/* batch frames of at most cap (<= 5632) keypoints each */
int aos2_frames_create(int device, int batch, int cap, aos2_frames_t **out);
void aos2_frames_destroy(aos2_frames_t *f);
void *aos2_frames_stream(aos2_frames_t *f);   /* the batch's hipStream_t */
/* Device-side ordering, no host wait: everything enqueued on the batch after this call runs behind the work enqueued on
 * `hip_stream` (a hipStream_t, NULL = the null stream) so far.  For the inputs the caller produces on a stream of its own:
 * the MapPoint table, d_local, d_Tcw, the depth images.  (The batches order themselves where they read each other:
 * aos2_frames_build behind the extractor's batch, aos2_frames_search_by_projection_last behind everything enqueued on
 * `last`'s stream -- in a tracking loop the previous CurrentFrame batch becomes LastFrame while its PoseOptimization is
 * still in flight.) */
int aos2_frames_wait_for_stream(aos2_frames_t *f, void *hip_stream);
/* waits for everything enqueued on the batch; AOS2_ERR_CAPACITY if a frame's search windows did not fit the entry pool */
int aos2_frames_wait(aos2_frames_t *f);

/* Frame::Frame(imGray, imDepth, ...)  src/Frame.cc:116-170, the part after ExtractORB: N = mvKeys.size(),
 * UndistortKeyPoints for a rectified / distortion-free camera (mvKeysUn = mvKeys, :436-442), ComputeStereoFromRGBD
 * (:672-693), mvpMapPoints = NULL, mvbOutlier = false, AssignFeaturesToGrid (:259-274); scale tables copied from the
 * extractor (:94-100).  d_kps / d_desc / d_n ([batch][cap], [batch][cap][32], [batch]) are the device outputs of `e`'s
 * last batch, which may still be in flight: the call orders itself behind it on the device and keeps referring to
 * these buffers (the caller keeps them alive and unchanged while the batch is used).
 * d_depth: `batch` float images (imDepth after convertTo(CV_32F, mDepthMapFactor), Tracking.cc:226-227), depth_stride
 * floats per row, depth_image_stride floats per image; NULL = monocular (mvuRight = mvDepth = -1). */
int aos2_frames_build(aos2_frames_t *f, aos2_extractor_t *e, int batch, const aos2_keypoint_t *d_kps,
                      const uint8_t *d_desc, const int32_t *d_n, int cap, int w, int h, const float *d_depth,
                      int depth_stride, size_t depth_image_stride, float fx, float fy, float cx, float cy, float mbf);
/* Frame::Frame(imLeft, imRight, ...)  src/Frame.cc:57-113, the part after the two ExtractORB calls and ComputeStereoMatches:
 * the same members as aos2_frames_build with mvuRight / mvDepth taken from d_u_right / d_depth_kp ([batch][cap], the device
 * outputs of aos2_compute_stereo_matches_device[_async] on `e_left`, which may still be in flight: the call orders itself
 * behind `e_left` on the device). */
int aos2_frames_build_stereo(aos2_frames_t *f, aos2_extractor_t *e_left, int batch, const aos2_keypoint_t *d_kps,
                             const uint8_t *d_desc, const int32_t *d_n, int cap, int w, int h, const float *d_u_right,
                             const float *d_depth_kp, float fx, float fy, float cx, float cy, float mbf);
/* mDistCoef (k1 k2 p1 p2 k3) for the following aos2_frames_build calls: with k1 != 0 (the reference's test, src/Frame.cc:435,
 * :467) mvKeysUn = cv::undistortPoints(mvKeys, K, mDistCoef, noArray(), K) and the image bounds are the undistorted corners
 * (Frame::UndistortKeyPoints / ComputeImageBounds :433-493); the depth map is still read at mvKeys (:678-683).  Default: 0. */
int aos2_frames_set_distortion(aos2_frames_t *f, float k1, float k2, float p1, float p2, float k3);
/* void Frame::ComputeImageBounds(const cv::Mat &imLeft)  src/Frame.cc:463-493 (once per camera: four points, host):
 * bounds4 = mnMinX mnMaxX mnMinY mnMaxY for a w x h image; dist5 = k1 k2 p1 p2 k3 */
int aos2_frame_image_bounds(int w, int h, float fx, float fy, float cx, float cy, const float *dist5, float *bounds4);
/* Frame::SetPose for every frame: d_Tcw = [batch][16] float32 in device memory (mVelocity * mLastFrame.mTcw, Tracking.cc:975).
 * Independent of aos2_frames_build (which leaves mTcw alone): called before it, the copy runs beside the extraction. */
int aos2_frames_set_pose(aos2_frames_t *f, const float *d_Tcw);
/* mvpMapPoints (and optionally mvbOutlier) from the host: mp = [batch][cap] rows of `table` (-1 = NULL), outlier =
 * [batch][cap] or NULL (unchanged); for setting up a LastFrame batch and tests */
int aos2_frames_set_map_points(aos2_frames_t *f, const int32_t *mp, const uint8_t *outlier,
                               const aos2_map_points_dev_t *table);
/* members back to the host (waits for the batch): */
#define AOS2_FRAMES_MAP_POINTS 0 /* int32 [batch][cap]  mvpMapPoints as table rows */
#define AOS2_FRAMES_OUTLIER 1    /* uint8 [batch][cap]  mvbOutlier */
#define AOS2_FRAMES_TCW 2        /* float [batch][16]   mTcw */
#define AOS2_FRAMES_U_RIGHT 3    /* float [batch][cap]  mvuRight */
#define AOS2_FRAMES_DEPTH 4      /* float [batch][cap]  mvDepth */
#define AOS2_FRAMES_GRID_OFF 5   /* int32 [batch][64 * 48 + 1]  mGrid as CSR */
#define AOS2_FRAMES_GRID_IDX 6   /* int32 [batch][cap] */
#define AOS2_FRAMES_KEYS_UN_X 7  /* float [batch][cap]  mvKeysUn[i].pt.x */
#define AOS2_FRAMES_KEYS_UN_Y 8  /* float [batch][cap]  mvKeysUn[i].pt.y */
#define AOS2_FRAMES_KEYS_ANGLE 9 /* float [batch][cap]  mvKeysUn[i].angle (= mvKeys[i].angle)   (device pointer only) */
#define AOS2_FRAMES_KEYS_OCTAVE 10 /* int32 [batch][cap] mvKeysUn[i].octave                      (device pointer only) */
int aos2_frames_get(aos2_frames_t *f, int what, void *dst, size_t bytes);
/* the member array itself in device memory ([batch][cap] ...), valid while the batch lives; NULL before the first build.
 * For handing Frame members to the other device-resident entry points (aos2_matcher_search_by_bow_device) without a copy;
 * the caller orders its reads behind the batch's stream (aos2_frames_wait or an event on aos2_frames_stream). */
const void *aos2_frames_device_ptr(aos2_frames_t *f, int what);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
 * src/ORBmatcher.cc:1328-1470 for the pairs (cur frame b, last frame b): reads last's mvpMapPoints / mvbOutlier /
 * mvKeys / mTcw and the table, writes cur's mvpMapPoints (the caller has just filled them with NULL,
 * Tracking.cc:977).  d_nmatches: [batch] return values in device memory, may be NULL.  The reference's retry with
 * 2 * th when fewer than 20 matches were found (Tracking.cc:984-988) is the caller's decision. */
int aos2_frames_search_by_projection_last(aos2_frames_t *cur, const aos2_frames_t *last,
                                          const aos2_map_points_dev_t *mps, float th, int mono,
                                          int check_orientation, int32_t *d_nmatches);
/* int Optimizer::PoseOptimization(Frame *pFrame)  src/Optimizer.cc:239-452 for every frame: edges from the features
 * that hold a map point (:260-350), result in mTcw and mvbOutlier; d_inliers [batch] (may be NULL) = return values */
/* (Two kernel forms: batches of more than 256 frames run 128 threads per frame with 9 edge slots each, smaller ones 256 threads
 * with 4; the edge order per thread and the order of the wave sums differ, so the SAME frame may get pose bits that differ in the
 * last places -- within 1e-5 of the oracle either way -- depending on the size of the batch it is in.  AOS2_PO_THREADS = 128 / 256
 * in the environment forces one form for every batch size.) */
int aos2_frames_pose_optimization(aos2_frames_t *f, const aos2_map_points_dev_t *mps, int32_t *d_inliers);
/* Tracking::TrackWithMotionModel :1008-1025 after PoseOptimization: a feature flagged as outlier loses its map point
 * (mvpMapPoints[i] = NULL, mvbOutlier[i] = false; the point counts as seen in this frame) */
int aos2_frames_discard_outliers(aos2_frames_t *f);
/* void Tracking::SearchLocalPoints()  src/Tracking.cc:1302-1352: d_local = [batch][n_local] rows of the table (-1 =
 * none) = mvpLocalMapPoints of every frame; points already in the frame are skipped (:1305-1328), the others go
 * through Frame::isInFrustum(pMP, 0.5) (src/Frame.cc:298-354) and ORBmatcher(nnratio).SearchByProjection(F,
 * vpMapPoints, th) (src/ORBmatcher.cc:45-129); writes mvpMapPoints.  At most 4096 features per frame. */
int aos2_frames_search_local_points(aos2_frames_t *f, const aos2_map_points_dev_t *mps, const int32_t *d_local,
                                    int n_local, float th, float nnratio, int32_t *d_nmatches);

/* Keyframe work on device-resident batches: a keyframe is a frame of a built batch (KeyFrame::KeyFrame copies exactly these
 * Frame members, src/KeyFrame.cc:37-62) with its mvpMapPoints set (aos2_frames_set_map_points or the tracking chain) and its
 * FeatureVector in HBM as aos2_vocabulary_transform_device wrote it.
 *
 * int ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)  src/ORBmatcher.cc:657-823 for n_pairs
 * (frame kf1[p] of `a`, frame kf2[p] of `b`) pairs -- LocalMapping::CreateNewMapPoints calls it once per neighbour keyframe
 * (src/LocalMapping.cc:272).  F12 (LocalMapping::ComputeF12) and the epipole (:663-670) are the caller's cv::Mat lines: host
 * arrays.  d_node_of1 = the node id of every feature of `a`'s frames at the FeatureVector level (aos2_vocabulary_transform_device's
 * d_node_of), d_fv_*1 / d_fv_*2 = the FeatureVectors of `a`'s / `b`'s frames (a feature whose word has weight 0 is in no
 * FeatureVector -- DBoW2 transform -- and the loop over KF1's FeatureVector never reaches it); all [batch][cap] device arrays
 * of the respective batch ([batch][cap + 1] for the offsets).
 * d_match12: DEVICE [n_pairs][cap of a] = vMatches12 (KF2 feature index or -1; vMatchedPairs = its non-negative entries in
 * ascending i), d_nmatches: DEVICE [n_pairs].  Returns when the results are complete. */
typedef struct {
    int32_t n_pairs;
    const int32_t *kf1, *kf2;      /* host [n_pairs] */
    const float *F12;              /* host [n_pairs][9], row-major */
    const float *epipole;          /* host [n_pairs][2]: ex, ey */
    const uint32_t *d_node_of1;
    const int32_t *d_fv_node1, *d_fv_off1, *d_fv_idx1, *d_n_fv1;
    const int32_t *d_fv_node2, *d_fv_off2, *d_fv_idx2, *d_n_fv2;
} aos2_frames_triang_t;
int aos2_frames_search_for_triangulation(aos2_frames_t *a, aos2_frames_t *b, const aos2_frames_triang_t *q,
                                         int only_stereo, int check_orientation, int32_t *d_match12,
                                         int32_t *d_nmatches);
/* The search part of int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th)  src/ORBmatcher.cc:825-975
 * for n_problems (target keyframe = frame target[p] of `kfs`, candidates = d_rows[p][0..n_pts): rows of the table, -1 where the
 * loop head rejects the point: NULL, isBad() or IsInKeyFrame(pKF) -- map state the caller evaluates) -- LocalMapping::
 * SearchInNeighbors calls it once per neighbour (src/LocalMapping.cc:493).  d_best_idx / d_best_dist: DEVICE [n_problems][n_pts]
 * as aos2_matcher_fuse returns them; the Replace / AddObservation bookkeeping of :948-969 consumes them on the host. */
int aos2_frames_fuse(aos2_frames_t *kfs, const aos2_map_points_dev_t *mps, int n_problems, int n_pts,
                     const int32_t *target, const int32_t *d_rows, float th, int32_t *d_best_idx,
                     int32_t *d_best_dist);
/* on != 0: aos2_frames_search_for_triangulation (handle = its `a`) and aos2_frames_fuse (handle = `kfs`) return after ENQUEUEING on the
 * handle's stream -- LocalMapping's three calls for a keyframe then cost one wait instead of three round trips through a device that
 * is busy with the tracking kernels; aos2_frames_wait(handle) (or ordering another stream behind aos2_frames_stream(handle))
 * completes them.  The host arrays of a call (kf1, kf2, F12, epipole, target) are copied before it returns; the OTHER handle of a call
 * (`b` of SearchForTriangulation, the keyframes a Fuse call reads) and every device input (the FeatureVector CSRs, d_node_of1, the map
 * point table) must stay untouched -- no rebuild, no set_pose, no reuse of the buffers -- until aos2_frames_wait(handle) of the handle
 * the call was made on has returned: its kernels read them from that handle's stream.  Default off: the calls return with their results
 * complete. */
int aos2_frames_set_async_keyframe_calls(aos2_frames_t *f, int on);

/* The loop body of void LocalMapping::CreateNewMapPoints()  src/LocalMapping.cc:290-436 for every matched pair: the parallax test
 * (:303-323), the linear triangulation (cv::SVD of the 4x4, :325-343), the KeyFrame::UnprojectStereo fallbacks (:344-351,
 * src/KeyFrame.cc:676-692) and the depth / reprojection / scale-consistency gates (:355-435) that decide whether a MapPoint is born.
 * `new MapPoint`, AddObservation and the rest of :438-453 stay with the caller.  What happened to a feature of keyframe 1: */
#define AOS2_TRI_NO_MATCH 0      /* match12 < 0, or a feature index >= N */
#define AOS2_TRI_ACCEPTED 1      /* x3D is a new map point */
#define AOS2_TRI_LOW_PARALLAX 2  /* no stereo and very low parallax (:352-353); also UnprojectStereo of a feature with mvDepth <= 0 */
#define AOS2_TRI_W_ZERO 3        /* x3D.at<float>(3) == 0 (:337) */
#define AOS2_TRI_DEPTH1 4        /* z1 <= 0 (:359) */
#define AOS2_TRI_DEPTH2 5        /* z2 <= 0 (:363) */
#define AOS2_TRI_REPROJ1 6       /* reprojection error in keyframe 1 (:372-391) */
#define AOS2_TRI_REPROJ2 7       /* reprojection error in keyframe 2 (:398-417) */
#define AOS2_TRI_ZERO_DIST 8     /* dist1 == 0 || dist2 == 0 (:426) */
#define AOS2_TRI_SCALE 9         /* scale consistency (:434) */
#define AOS2_TRI_SUPERSEDED 10   /* passed every gate, but an earlier pair of the same keyframe 1 created the feature's point (first_wins) */
/* Device-resident form, for n_pairs (frame kf1[p] of `a`, frame kf2[p] of `b`) pairs and the d_match12 that
 * aos2_frames_search_for_triangulation wrote for them (vMatchedIndices = its non-negative entries).  The two batches may have
 * different cameras; the mbf of the stereo reprojection term is keyframe 1's in both keyframes, as in :384 and :410.
 * first_wins != 0 restores the coupling between the neighbours of one keyframe that a batched search at one snapshot cannot have:
 * the reference searches neighbour p + 1 after the points of neighbour p were added, and SearchForTriangulation skips a feature of
 * keyframe 1 that holds a map point (src/ORBmatcher.cc:700-703).  The pairs of the call that share kf1 are one CreateNewMapPoints
 * call, in call order = neighbour order: the first accepted pair of a feature keeps it, later accepted ones become
 * AOS2_TRI_SUPERSEDED (exact, because the features of keyframe 1 are searched independently: vbMatched2 is never set).
 * d_x3D: DEVICE [n_pairs][cap of a][3], defined where the status is not 0, 2 or 3 (zeros there); d_status: DEVICE [n_pairs][cap of a];
 * d_nnew: DEVICE [n_pairs] = entries with status 1 (nnew, :453).  Pairs outside the batches are rejected with AOS2_ERR_ARG before
 * anything runs.  Ordered behind b's stream; with aos2_frames_set_async_keyframe_calls(a, 1) it returns after enqueueing (kf1 / kf2
 * are copied before it returns; its staging buffer is its own, so the three keyframe calls of a handle may all be in flight). */
int aos2_frames_triangulate_matches(aos2_frames_t *a, aos2_frames_t *b, int n_pairs, const int32_t *kf1, const int32_t *kf2,
                                    const int32_t *d_match12, int first_wins, float *d_x3D, uint8_t *d_status,
                                    int32_t *d_nnew);
/* Host-pointer form for ONE (KF1, KF2) pair and its n matches (the shim's route, host/NewMapPoints.h): the members the loop reads */
typedef struct {
    float Tcw1[16], Tcw2[16];                       /* mTcw of both keyframes, row-major 4x4 */
    float fx1, fy1, cx1, cy1, mb1, mbf1;            /* mpCurrentKeyFrame */
    float fx2, fy2, cx2, cy2, mb2, mbf2;            /* pKF2 */
    int32_t n_levels;                               /* <= 8 */
    float scale_factors1[8], scale_factors2[8];     /* mvScaleFactors (mvLevelSigma2 = their squares, ORBextractor.cc:420) */
} aos2_triang_geom_t;
typedef struct {
    float ux, uy;      /* mvKeysUn[i].pt */
    float kx, ky;      /* mvKeys[i].pt (KeyFrame::UnprojectStereo reads the distorted key) */
    float u_right;     /* mvuRight[i] */
    float depth;       /* mvDepth[i] */
    int32_t octave;    /* mvKeysUn[i].octave */
} aos2_triang_obs_t;
/* obs1 / obs2: host [n], match k = (feature of KF1, feature of KF2); x3D: host [n][3], status: host [n] (never 0 or 10) */
int aos2_triangulate_matches(aos2_matcher_t *m, const aos2_triang_geom_t *g, int n, const aos2_triang_obs_t *obs1,
                             const aos2_triang_obs_t *obs2, float *x3D, uint8_t *status);

/* ------------------------------------------------------------------------------------------
 * Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) and the tail of Tracking::TrackLocalMap (:1040-1071) for frame batches
 * (csrc/local_map.hip): the first line of TrackLocalMap decides what SearchLocalPoints searches, from the mvpMapPoints that
 * SearchByProjection(Cur, Last), PoseOptimization and the outlier discard have just left on the device.  A handle keeps a
 * snapshot of the parts of Map that UpdateLocalMap reads -- the covisibility graph -- in HBM; the call writes mvpLocalMapPoints
 * of every frame straight into the d_local that aos2_frames_search_local_points reads, with no host wait in between.
 * Integer graph work, no floating point: the results are a function of the frame and the graph alone.
 *
 * Conventions: the reference walks map<KeyFrame*, int>, map<KeyFrame*, size_t> and set<KeyFrame*>
 * in pointer order, an accident of the allocator; here ASCENDING KEYFRAME ROW stands for it (the vote map, the observations and
 * the children).  Everything else is followed literally.
 * ------------------------------------------------------------------------------------------ */
typedef struct aos2_local_map aos2_local_map_t;
#define AOS2_LOCAL_MAP_NEIGHBOURS 10   /* GetBestCovisibilityKeyFrames(10) :1470 */
#define AOS2_LOCAL_MAP_MAX_KFS 80      /* mvpLocalKeyFrames.size() > 80 :1465 */
/* Host arrays; point rows are the rows of the caller's aos2_map_points_dev_t table, keyframe rows are the caller's (the host
 * class uses ascending mnId).  Offsets are CSR: off[0] = 0, off[i + 1] - off[i] entries of row i. */
typedef struct {
    int32_t n_points;
    const uint8_t *point_bad;      /* [n_points]      MapPoint::isBad() */
    const int32_t *point_nobs;     /* [n_points]      MapPoint::Observations() = nObs: a stereo observation counts twice, so this
                                                      is not the length of the list below */
    const int32_t *obs_off;        /* [n_points + 1]  MapPoint::GetObservations(): the keyframe rows of each point, each keyframe */
    const int32_t *obs_kf;         /*                 at most once per point (a map has one entry per key) */
    int32_t n_keyframes;
    const uint8_t *kf_bad;         /* [n_keyframes]      KeyFrame::isBad() */
    const int32_t *kf_mp_off;      /* [n_keyframes + 1]  KeyFrame::GetMapPointMatches(): one entry per feature, in feature order, */
    const int32_t *kf_mp;          /*                    -1 = NULL */
    const int32_t *kf_best;        /* [n_keyframes][10]  GetBestCovisibilityKeyFrames(10), in its order, padded with -1 */
    const int32_t *kf_child_off;   /* [n_keyframes + 1]  KeyFrame::GetChilds() (any order: walked in ascending row) */
    const int32_t *kf_child;
    const int32_t *kf_parent;      /* [n_keyframes]      KeyFrame::GetParent(), -1 = none */
} aos2_local_map_graph_t;

int aos2_local_map_create(int device, aos2_local_map_t **out);
void aos2_local_map_destroy(aos2_local_map_t *m);
/* Replaces the handle's snapshot (Map::GetAllKeyFrames / GetAllMapPoints with the members above, as Tracking reads them under
 * mMutexMapUpdate) and uploads it; returns when the upload is complete.  The graph is checked BEFORE a device is looked for:
 * AOS2_ERR_ARG, with the handle's previous graph left in place, for a negative count, an array that is NULL with a non-zero
 * count, offsets that do not start at 0 or that decrease, a row out of range (other than the -1 the members allow) and a
 * keyframe listed twice among one point's observations.  An empty map (0 keyframes, 0 points) is valid.  A graph that passed the
 * check is the handle's from then on, also when the upload fails (AOS2_ERR_NO_DEVICE, AOS2_ERR_HIP): the next
 * aos2_frames_update_local_map uploads it.  The whole graph is sent every time; aos2_local_map_apply (below) changes a resident
 * graph by one keyframe's worth of rows without re-sending the rest. */
int aos2_local_map_set(aos2_local_map_t *m, const aos2_local_map_graph_t *g);
/* the handle's snapshot: its sizes and, in *g (may be NULL), its arrays (the handle's own copies, valid until the next set or
 * apply; behind an aos2_local_map_apply that ran on the device the first call downloads them, AOS2_ERR_HIP if that fails) */
int aos2_local_map_get(const aos2_local_map_t *m, aos2_local_map_graph_t *g);

/* void Tracking::UpdateLocalMap() = UpdateLocalKeyFrames() (:1411-1519) + UpdateLocalPoints() (:1385-1408) for every frame of
 * the batch, enqueued on the batch's stream, no host wait.  The frames' mvpMapPoints are rows of the graph's point table.
 * Device arrays: d_local [batch][local_cap] = mvpLocalMapPoints, d_n_local [batch]; d_local_kfs [batch][kf_cap] =
 * mvpLocalKeyFrames, d_n_local_kfs [batch], d_ref_kf [batch] = mpReferenceKF -- these three are IN / OUT.
 *   :1415-1431  a feature whose point isBad() loses it (the batch's mvpMapPoints[i] = -1: a write to the batch); every other
 *               matched feature votes once for each keyframe of its point's observations
 *   :1433       no votes: the function returns, and UpdateLocalPoints still runs over the PREVIOUS mvpLocalKeyFrames: the three
 *               in / out arrays of that frame are left exactly as passed and the points are gathered from its first
 *               min(n, kf_cap) rows (rows outside the graph are skipped).  A caller without a previous list passes n = 0.
 *   :1443-1458  the keyframes with votes in ascending row, bad ones skipped; mpReferenceKF = the first of them with strictly
 *               more votes than every one before it.  All of them bad: the list is empty, d_ref_kf unchanged.
 *   :1462-1512  for the keyframes of that first pass only, and only while the list holds at most 80: the first of the 10 best
 *               covisibles that is not bad and not in the list; the first child, in ascending row, that is not bad and not in
 *               the list; the parent if it is not in the list -- NOT tested for isBad, and adding it ends the whole loop.
 *   :1385-1408  the local keyframes in list order, their matches in feature order: NULL and bad points skipped, a point kept at
 *               its first occurrence only.  (A point the frame holds is listed: SearchLocalPoints skips it.)
 * d_n_local and d_n_local_kfs are the true counts; rows from the count to the capacity are -1 (d_local goes into
 * aos2_frames_search_local_points with n_local = local_cap as it is).  A count above its capacity: the first `cap` rows are
 * written, nothing behind the array is touched, and the points still come from the whole keyframe list (kept in the handle's
 * scratch).  A feature whose row is outside the table (>= n_points) is left alone and does not vote.
 * Scratch is bounded: 4 (n_points + 2 n_keyframes) bytes per frame, the frames of a batch run in
 * groups that fit 256 MiB, one after the other on the stream; a graph of which ONE frame does not fit is refused with
 * AOS2_ERR_ARG before anything is enqueued.  Concurrent calls with one handle share that scratch: one stream at a time. */
int aos2_frames_update_local_map(aos2_frames_t *f, const aos2_local_map_t *m, int32_t *d_local, int local_cap, int32_t *d_n_local,
                                 int32_t *d_local_kfs, int kf_cap, int32_t *d_n_local_kfs, int32_t *d_ref_kf);
/* Host-pointer form (the route of host/LocalMap.h, for a tracker whose Frames live on the host): n [batch] = Frame::N, mp
 * [batch][cap] = mvpMapPoints as rows (in / out), the five arrays as above, all HOST memory; copied to the device, the same
 * kernels on the handle's own stream, copied back; returns when the results are complete. */
int aos2_local_map_update(aos2_local_map_t *m, int batch, int cap, const int32_t *n, int32_t *mp, int32_t *local, int local_cap,
                          int32_t *n_local, int32_t *local_kfs, int kf_cap, int32_t *n_local_kfs, int32_t *ref_kf);
/* The tail of bool Tracking::TrackLocalMap() (:1040-1071) for every frame, after the second PoseOptimization:
 * d_stats [batch][3] = nObsvMappoints, mnMatchesInliers, totalObservation (Observations() = the graph's point_nobs; with
 * only_tracking = mbOnlyTracking every inlier counts and totalObservation stays 0, :1053-1061); with stereo (mSensor ==
 * System::STEREO) a feature flagged as outlier loses its point (:1063-1064: a write to the batch; mvbOutlier stays).
 * d_found_inc [n_points] or NULL: MapPoint::IncreaseFound() as integer atomic adds ON TOP of what the array holds (the caller
 * zeroes it).  IncreaseVisible and the mnLastFrameSeen bookkeeping of SearchLocalPoints (:1305-1345) stay with the caller. */
int aos2_frames_track_local_map_stats(aos2_frames_t *f, const aos2_local_map_t *m, int stereo, int only_tracking, int32_t *d_stats,
                                      int32_t *d_found_inc);
/* test hooks: the scratch bound in bytes (<= 0: the default, 256 MiB) and the largest n_keyframes whose vote counters live in
 * LDS (< 0: the default, 8192; 0: always global memory), so that both sides of either switch are reached with small graphs */
int aos2_local_map_debug_limits(aos2_local_map_t *m, int64_t scratch_bytes, int lds_keyframes);
/* groups the last aos2_frames_update_local_map, aos2_local_map_update_connections or aos2_local_map_update_normal_depth call ran
 * its batch in */
int aos2_local_map_last_groups(const aos2_local_map_t *m);

/* ------------------------------------------------------------------------------------------
 * LocalMapping::KeyFrameCulling (src/LocalMapping.cc:636-700, called at :87) over the handle's resident graph
 * (csrc/kf_culling.hip): for every covisible keyframe of the new keyframe, nMPs and nRedundantObservations, the cull test, and --
 * because the loop is serial in its effects -- what KeyFrame::SetBadFlag (src/KeyFrame.cc:514-532) of every culled keyframe does
 * to the candidates behind it: MapPoint::EraseObservation (src/MapPoint.cc:144-170) on each of its points, and the points that
 * fall to nObs <= 2 and go bad.  Integer graph work.  The resident graph is READ, never written: the caller applies the verdicts
 * to its own map (SetBadFlag in candidate order) and sends the result as a delta (aos2_local_map_apply), as after every other map change.
 *
 * Followed literally: the far-point gate `mvDepth[i] > mThDepth || mvDepth[i] < 0` as float compares
 * when not monocular; Observations() > 3 on nObs (a stereo observation counts twice); the observer count over observation
 * entries with pKFi == pKF skipped, the gate scaleLeveli <= scaleLevel + 1 and the stop at 3; the test nRedundantObservations >
 * 0.9 * nMPs as an int against a double product; no isBad() test on the candidate.  The reference walks the observations in
 * pointer order; the count stops at 3 whichever entries come first, so NO ordering convention is involved here.
 * ------------------------------------------------------------------------------------------ */
/* What the loop reads beside the graph.  The arrays are parallel to the graph's own, so their lengths are the graph's. */
typedef struct {
    const int32_t *obs_idx;      /* parallel to obs_kf: mit->second, the feature of that keyframe that observes the point */
    const int8_t  *kf_octave;    /* parallel to kf_mp: mvKeysUn[i].octave */
    const float   *kf_depth;     /* parallel to kf_mp: mvDepth[i] */
    const uint8_t *kf_stereo;    /* parallel to kf_mp: mvuRight[i] >= 0 */
    const float   *kf_th_depth;  /* [n_keyframes] mThDepth */
    const uint8_t *kf_flags;     /* [n_keyframes] bit 0: mnId == 0, bit 1: mbNotErase */
} aos2_kf_culling_view_t;
#define AOS2_KFC_KEPT 0      /* not redundant */
#define AOS2_KFC_CULLED 1    /* SetBadFlag erases the keyframe */
#define AOS2_KFC_DEFERRED 2  /* SetBadFlag with mbNotErase: mbToBeErased is set, nothing is erased, later candidates see no change */
#define AOS2_KFC_SKIPPED 3   /* mnId == 0 (:647) */
/* Checks the view against the handle's graph, keeps a copy and uploads it; returns when the upload is complete.  AOS2_ERR_ARG
 * BEFORE a device is looked for, with the handle's previous view left in place: no graph has been set, an array is NULL while
 * the graph gives it a non-zero length, an obs_idx outside the feature range of its keyframe.  As with aos2_local_map_set, a view
 * that passed is the handle's also when the upload fails (AOS2_ERR_NO_DEVICE, AOS2_ERR_HIP): the culling call uploads it.  A later
 * aos2_local_map_set DROPS the view: its arrays no longer line up with the graph. */
int aos2_local_map_set_culling_view(aos2_local_map_t *m, const aos2_kf_culling_view_t *view);
/* The loop :644-699.  cand [n_cand] = the rows of mpCurrentKeyFrame->GetVectorCovisibleKeyFrames() in its order; monocular =
 * mbMonocular.  All arrays are HOST memory; the call returns when the results are complete.  AOS2_ERR_ARG before any device work:
 * no view, n_cand < 0, a NULL array with n_cand > 0, n_bad_points NULL, bad_cap < 0 (or > 0 with bad_points NULL), a row out of
 * range, a row listed twice, and a map whose overlay exceeds the handle's scratch bound (13 bytes per point + 1 per observation
 * against the 256 MiB of aos2_local_map_debug_limits).  n_cand == 0 is valid.
 * Per candidate, in the loop's order: status [n_cand] = AOS2_KFC_*; n_mps / n_redundant [n_cand] = nMPs and
 * nRedundantObservations as the serial loop has them when it reaches that candidate, AFTER the effects of every earlier cull (0 for
 * a skipped candidate).  A CULLED candidate c changes the rest of the call, one effect per point however often the point sits among
 * c's matches: for each non-NULL match, bad or not, whose observations contain c that entry is gone and nObs drops by 2 if
 * kf_stereo at the OBSERVATION's feature of c is set, by 1 otherwise; with nObs <= 2 the point is bad from then on and every
 * later candidate skips it; a match whose point does not list c changes nothing (and an entry of c in the observations of a point
 * that c does not hold stays).  DEFERRED and KEPT change nothing.
 * bad_points (may be NULL with bad_cap 0): the rows of the points that went bad DURING the call (not those the graph already
 * marks), ascending; *n_bad_points is the true count, the first min(count, bad_cap) are written, nothing behind them.
 * The work runs in rounds, culls + 1 of them; the outputs do not depend on how many one enqueue holds.
 * It runs on the handle's own stream and shares the handle's scratch with aos2_local_map_update: one call at a time. */
int aos2_local_map_keyframe_culling(aos2_local_map_t *m, int monocular, int n_cand, const int32_t *cand, uint8_t *status,
                                    int32_t *n_mps, int32_t *n_redundant, int32_t *bad_points, int bad_cap, int32_t *n_bad_points);
/* test hooks: the rounds (count + apply launches) one enqueue holds (<= 0: the default, 4), and the rounds the last call needed */
int aos2_local_map_debug_culling_rounds(aos2_local_map_t *m, int rounds);
int aos2_local_map_last_culling_rounds(const aos2_local_map_t *m);
/* device time of the last aos2_local_map_keyframe_culling call between two events on the handle's stream, from the upload of the
 * candidates to the last copy back (the host's waits between enqueues included); -1 if there was none */
float aos2_local_map_last_culling_device_ms(aos2_local_map_t *m);
/* the handle's view in *view (the handle's own copies, parallel to the arrays of aos2_local_map_get and valid as long as they are);
 * *has_view (may be NULL) = whether the handle holds one, every pointer NULL if not */
int aos2_local_map_get_culling_view(const aos2_local_map_t *m, aos2_kf_culling_view_t *view, int32_t *has_view);

/* ------------------------------------------------------------------------------------------
 * KeyFrame::UpdateConnections (src/KeyFrame.cc:350-440; called at LocalMapping.cc:168 and :537, Tracking.cc:775-776,
 * LoopClosing.cc:434, :517, :556) over the handle's resident graph (csrc/connections.hip): the counting stage and the ordering,
 * for a batch of keyframes in one call.  Every keyframe of the batch is independent: the counting stage reads points and
 * observations, never connection weights, so the sequential loops of CorrectLoop are exact as one batch.  Integer graph work.
 * The resident graph is READ, never written: the caller applies the verdicts to its own pointer graph (AddConnection on the
 * neighbours, the three members, the first-connection parent: host/UpdateConnections.h) and sends the new link rows with its
 * next aos2_local_map_apply.
 *
 * Followed literally, per keyframe k:
 *   :363-381  every entry of the matches in feature order; a NULL (-1) entry and a point with isBad() are skipped; every
 *             observation of the point whose keyframe is not k counts once for that keyframe.  No isBad() test on the observer or
 *             on k; a point that sits at two features counts twice.
 *   :384      no counter: the keyframe's members stay as they are.  n_conn = 0, n_ordered = 0.
 *   :389-413  every counter >= th is listed (th: the reference's literal 15, AOS2_CONNECTIONS_TH); if none is, the single pKFmax =
 *             the first strict maximum in the map's iteration order = the LOWEST row among the keyframes of maximal weight
 *             (ascending row stands for pointer order).
 *   :415-422  the list sorted on (weight, KeyFrame*) ascending and reversed: DESCENDING weight, and among equal weights
 *             DESCENDING row -- not the order of the line above.
 *   :428-430  mConnectedKeyFrameWeights = every keyframe with a count > 0, below the threshold or not.
 * ------------------------------------------------------------------------------------------ */
#define AOS2_CONNECTIONS_TH 15
/* kf [n] = the keyframe rows.  All arrays are HOST memory; the call runs on the handle's own stream, shares the handle's scratch
 * with aos2_local_map_update and aos2_local_map_keyframe_culling (one call at a time) and returns when the results are complete.
 * Matches: with n_mp, mp and mp_cap NULL / NULL / 0 they are the resident kf_mp row of kf[k], which must be a row of the graph.
 * With mp [n][mp_cap] and n_mp [n] given they are mp[k][0 .. n_mp[k]), 0 <= n_mp[k] <= mp_cap; kf[k] then only names the observer
 * to skip and may be -1, a keyframe the graph does not know yet: nothing is skipped (the form for LocalMapping.cc:168).  An entry
 * >= n_points is a point the table does not know and is skipped, as aos2_frames_update_local_map skips one.  A row may be listed
 * twice in a batch; n == 0 is valid.
 * Outputs: n_conn [n] / n_ordered [n] = the true counts; conn_kf / conn_w [n][conn_cap] = KFcounter in ascending row; ordered_kf /
 * ordered_w [n][ordered_cap] = mvpOrderedConnectedKeyFrames / mvOrderedWeights.  The first min(count, cap) entries of a row are
 * written, entries from the count to the capacity are -1 (keyframe) and 0 (weight), nothing behind an array is touched.  A
 * capacity of 0 with NULL arrays is valid: the counts are still returned.
 * AOS2_ERR_ARG before a device is looked for: no graph set; th < 1; a negative count or capacity; a NULL array with a non-zero
 * length; mp without n_mp or the reverse; a row out of range; an n_mp[k] outside [0, mp_cap]; a match entry < -1; a scratch need of
 * ONE keyframe (12 n_keyframes + 16 bytes: DESIGN.md section 5.16) above the bound of aos2_local_map_debug_limits.  A batch runs
 * in groups that fit that bound (aos2_local_map_last_groups counts them); the outputs do not depend on the grouping, on where the
 * counters live or on where the list is sorted.  After an aos2_local_map_apply that ran on the device the call reads the new block.
 * Without a device: AOS2_ERR_NO_DEVICE. */
int aos2_local_map_update_connections(aos2_local_map_t *m, int th, int n, const int32_t *kf, const int32_t *n_mp, const int32_t *mp,
                                      int mp_cap, int32_t *n_conn, int32_t *conn_kf, int32_t *conn_w, int conn_cap, int32_t *n_ordered,
                                      int32_t *ordered_kf, int32_t *ordered_w, int ordered_cap);
/* device time of the last aos2_local_map_update_connections call between two events on the handle's stream, from the upload of
 * the arguments to the copy back; -1 if there was none */
float aos2_local_map_last_connections_device_ms(aos2_local_map_t *m);
/* test hook: the longest ordered list that is sorted in LDS (<= 0: the default, 2048, which is also the most), so that the form
 * in global scratch is reached with small graphs */
int aos2_local_map_debug_connections_sort(aos2_local_map_t *m, int lds_entries);

/* ------------------------------------------------------------------------------------------
 * MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:363-413 with compute_std_pts :27-37; called at LocalMapping.cc:156, :448, :531,
 * Tracking.cc:628, :764, :1298, Optimizer.cc:227, :777, :1043, LoopClosing.cc:502) for a batch of points over the handle's resident
 * observation lists (csrc/normal_depth.hip): mNormalVector, mfMinDistance, mfMaxDistance, theta_mean and theta_std, the
 * per-observation mNormalVectors / theta_sVector, and the planner's map rows that Planning.cc:86-96 and Tracking.cc:1088-1112 derive
 * from them.  The observers and their feature indices are the resident obs_kf rows and the culling view's obs_idx / kf_octave;
 * the geometry (point positions, camera centres, the scale table) comes in with the call.  The resident graph is READ, never written.
 *
 * Conventions (parity unpinned: the cv::Mat expressions are restated as OpenCV 3.2's plain path):
 * the observers are taken in the STORED order of the point's observation row (the host class stores ascending keyframe row, which
 * stands for pointer order as in items 18 and 20); every sum is folded in that order, one add after the other.  Per observation k:
 * d = P - O_k in float; nrm = sqrt(((double)d0 d0 + (double)d1 d1) + (double)d2 d2) in double (cv::norm); u = d * (float)(1.0 / nrm);
 * normal += u in float from 0; theta = (float)atan2((double)d0, (double)d2).  Behind the loop, n = the length of the list:
 * mNormalVector = normal * (float)(1.0 / (double)n); dist = (float)nrm over P - O_ref; level = kf_octave of feature
 * observations[pRefKF] of the reference keyframe (feature 0 if it does not observe the point: what map::operator[] yields);
 * mfMaxDistance = dist * scale[level]; mfMinDistance = mfMaxDistance / scale[n_levels - 1]; compute_std_pts literally: a double
 * accumulator over the float thetas rounded to float, mean = sum / (float)n, a double accumulator over the FLOAT products
 * (theta - mean)^2 rounded to float, std = sqrtf(sq / (float)n).  A point on a camera centre gives NaN where the reference does.
 * ------------------------------------------------------------------------------------------ */
#define AOS2_ND_UPDATED 0        /* the members were written */
#define AOS2_ND_BAD 1            /* isBad(): the return at :371 */
#define AOS2_ND_NO_OBS 2         /* no observation: the return at :378 */
#define AOS2_ND_UNKNOWN 3        /* a point row >= n_points: a point the table does not know */
#define AOS2_ND_REF_UNUSABLE 4   /* the reference keyframe has no feature, or the octave is outside [0, n_levels): the reference
                                    reads out of bounds there */
#define AOS2_ND_ROWS_PLANNING 0  /* Planning.cc:86-93: theta_interval is a float member, floor 30.0 / 57.3 */
#define AOS2_ND_ROWS_TRACKING 1  /* Tracking.cc:1103-1110: theta_interval is a double local, floor 10.0 / 57.3 */
/* One call's arguments, all HOST memory. */
typedef struct {
    int32_t n;
    const int32_t *point;      /* [n]     the point rows; a row may repeat, a row >= n_points is skipped (AOS2_ND_UNKNOWN) */
    const float *xyz;          /* [n][3]  mWorldPos of each listed point */
    const int32_t *ref_kf;     /* [n]     the row of mpRefKF */
    const float *kf_center;    /* [n_keyframes][3]  GetCameraCenter() of every keyframe row of the graph */
    int32_t n_levels;
    const float *scale;        /* [n_levels]  mvScaleFactors (one table for every keyframe) */
    int32_t rows_form;         /* AOS2_ND_ROWS_* : the form of upper / lower */
    const int32_t *term_off;   /* [n + 1] or NULL: where the per-observation outputs of each listed point go (CSR) */
    /* outputs, each may be NULL = not wanted.  status is written for every listed point; every other output of a point whose
     * status is not AOS2_ND_UPDATED is left untouched, as the reference leaves the members */
    uint8_t *status;           /* [n]     AOS2_ND_* */
    float *normal;             /* [n][3]  mNormalVector */
    float *min_dist, *max_dist, *theta_mean, *theta_std;   /* [n] */
    int32_t *n_terms;          /* [n]     the true length of the observation list */
    float *upper, *lower;      /* [n]     theta_mean +- theta_interval in the form of rows_form */
    float *max_range, *min_range;   /* [n]  GetMaxDistanceInvariance() = 1.2f max, GetMinDistanceInvariance() = 0.8f min */
    /* mNormalVectors [term_off[n]][3] and theta_sVector [term_off[n]] in list order: written only for the points where
     * term_off[i + 1] - term_off[i] equals the list length */
    float *term_unit, *term_theta;
} aos2_normal_depth_t;
/* Runs on the handle's own stream, shares the handle's scratch with the other aos2_local_map_* calls (one call at a time) and
 * returns when the results are complete.  n == 0 is valid.
 * AOS2_ERR_ARG before a device is looked for: no graph set; no culling view set; a negative count; n_levels < 1; point, xyz,
 * ref_kf, kf_center or scale NULL with a non-zero length; a ref_kf outside [0, n_keyframes); a point row < 0; term_off that does not
 * start at 0 or that decreases; term_unit or term_theta without term_off; an unknown rows_form; ONE observation list whose thetas
 * need more scratch than the bound of aos2_local_map_debug_limits (4 bytes per observation of a list longer than the LDS form
 * holds: DESIGN.md section 5.17).  A batch runs in groups that fit that bound (aos2_local_map_last_groups counts them); the outputs
 * do not depend on the grouping or on where the thetas wait between the two passes of compute_std_pts.  After an
 * aos2_local_map_apply that ran on the device the call reads the new block.  Without a device: AOS2_ERR_NO_DEVICE. */
int aos2_local_map_update_normal_depth(aos2_local_map_t *m, const aos2_normal_depth_t *a);
/* device time of the last aos2_local_map_update_normal_depth call between two events on the handle's stream, from the upload of
 * the arguments to the copy back; -1 if there was none (a call with n == 0 included) */
float aos2_local_map_last_normal_depth_device_ms(aos2_local_map_t *m);
/* test hook: the longest observation list whose thetas wait in LDS (< 0: the default, 64, which is also the most; 0: every list
 * waits in global scratch), so that both forms and the groups are reached with small inputs */
int aos2_local_map_debug_normal_depth(aos2_local_map_t *m, int lds_terms);

/* ------------------------------------------------------------------------------------------
 * One keyframe's changes applied to the resident graph (csrc/local_map_apply.hip): what one pass of
 * LocalMapping::Run (src/LocalMapping.cc:49-107) does to the map -- a keyframe inserted, points created, culled and fused,
 * covisibility lists and the spanning tree re-linked, keyframes culled -- touches a few hundred rows of 10^5.  The delta names
 * those rows and carries their new content; the new arrays are built ON THE DEVICE from the resident graph and the delta, and
 * the culling view moves with the graph.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    /* counts AFTER the delta; rows only ever get appended */
    int32_t n_points, n_keyframes;
    /* point rows replaced wholesale (strictly ascending): isBad, nObs, the observation list */
    int32_t n_point_rows;   const int32_t *point_row;
    const uint8_t *point_bad;  const int32_t *point_nobs;           /* [n_point_rows] */
    const int32_t *obs_off, *obs_kf;                                /* CSR over the n_point_rows rows */
    /* keyframe MATCH rows replaced wholesale (strictly ascending): GetMapPointMatches() */
    int32_t n_kf_mp_rows;   const int32_t *kf_mp_row;
    const int32_t *kf_mp_off, *kf_mp;                               /* CSR over the n_kf_mp_rows rows */
    /* keyframe LINK rows replaced wholesale (strictly ascending): isBad, the 10 best covisibles, children, parent */
    int32_t n_kf_link_rows; const int32_t *kf_link_row;
    const uint8_t *kf_bad;  const int32_t *kf_best /* [rows][10] */, *kf_child_off, *kf_child, *kf_parent;
    /* NULL if and only if the handle holds no culling view.  Parallel to the delta's arrays: obs_idx to obs_kf;
     * kf_octave / kf_depth / kf_stereo to kf_mp; kf_th_depth / kf_flags [n_kf_link_rows] */
    const aos2_kf_culling_view_t *view;
} aos2_local_map_delta_t;
/* The graph after the call is the graph before it with every named row replaced by the delta's content and the tables extended
 * to the new counts.  An appended point row that the delta does not name is an empty slot (bad = 1, nObs = 0, no observations);
 * an appended keyframe row must be named in BOTH keyframe row sets.  Child lists are stored in ascending row, as
 * aos2_local_map_set stores them.  An empty delta is valid and changes nothing; a handle without a set holds the empty map (and
 * no view), and a delta may be applied to it.  The culling view is NOT dropped: it moves with the graph.
 * Checked BEFORE a device is looked for, in O(delta) against counts the handle keeps on the host -- AOS2_ERR_ARG with the graph
 * and the view left exactly as they were for: a NULL handle or delta; a count below the current one; a row list that is not
 * strictly ascending or holds a row outside the new count; an appended keyframe missing from either keyframe set; a NULL array
 * with a non-zero length (an offsets array of a row set without rows may be NULL); offsets that do not start at 0 or that
 * decrease; a value outside the new counts (other than the -1 that kf_mp, kf_best and kf_parent allow); a keyframe listed twice
 * among one point's observations; a match row of an EXISTING keyframe whose length differs from the one it has (a keyframe's N
 * never changes: that keeps the obs_idx of untouched points in range); `view` given without a resident view, or missing with
 * one; an obs_idx outside the feature count its keyframe has after the delta; more than 2^31 - 1 entries in an array.
 * Where the work runs: with the graph (and the view, if there is one) resident, only the delta is uploaded and the new arrays
 * are built by kernels on the handle's stream into the second of two device blocks; on an allocation or HIP failure
 * (AOS2_ERR_HIP) the previous block stays current and the graph is unchanged.  The handle's host copy then goes stale and is
 * refreshed by ONE download when something next reads it (aos2_local_map_get, aos2_local_map_get_culling_view, the check of
 * aos2_local_map_set_culling_view, a re-upload).  With the graph not resident (no device, or never uploaded) the same rebuild
 * runs serially on the host copy and the return value follows aos2_local_map_set: AOS2_OK or AOS2_ERR_NO_DEVICE, and a delta
 * that passed the check is the handle's either way.
 * Ordering: as aos2_local_map_set.  The call synchronises the device before it builds the new block, and returns when the new
 * graph is complete: work enqueued before the call sees the old graph, work enqueued after it the new one.  Removing that wait
 * (an event per consumer stream) is out of scope. */
int aos2_local_map_apply(aos2_local_map_t *m, const aos2_local_map_delta_t *d);
/* the last aos2_local_map_apply that passed its checks: *path = 0 host, 1 device (-1: none yet); *reallocated = the device block
 * it wrote had to be allocated or grown (blocks grow with a quarter of slack); *device_ms = between two events on the handle's
 * stream, from the delta's upload to the last kernel (-1 on the host path).  Any of the three may be NULL. */
int aos2_local_map_last_apply(const aos2_local_map_t *m, int32_t *path, int32_t *reallocated, float *device_ms);
/* bytes the last device rebuild uploaded (0 on the host path) */
int64_t aos2_local_map_last_apply_bytes(const aos2_local_map_t *m);
/* test hook: the rows one workgroup scans in the rebuild (<= 0: the default, 1024), so that the seams of the multi-workgroup scan
 * and the loop over the workgroups' totals are reached with graphs of a few hundred rows */
int aos2_local_map_debug_apply_tile(aos2_local_map_t *m, int rows);

/* ------------------------------------------------------------------------------------------
 * Replay of a fixed call sequence (csrc/replay.hip).  No single reference function: the per-frame body of Tracking::Track on its
 * usual path -- Frame::Frame (src/Frame.cc:116-172), TrackWithMotionModel (src/Tracking.cc:860-1039: SearchByProjection,
 * PoseOptimization, the outlier discard), TrackLocalMap (:1041-1100: SearchLocalPoints, PoseOptimization) -- is the same ~20
 * dependent launches for every frame.  For one sequence (batch 1) the launches' own latency is a sixth of the frame time; a
 * recorded sequence is enqueued with one call and its kernels run back to back.
 *
 *   run the sequence once (the handles allocate on their first call with a shape), then
 *   aos2_capture_begin(aos2_frames_stream(cur));
 *   aos2_extractor_wait_for_stream(e, aos2_frames_stream(cur));      -- the extractor's stream joins the recording
 *   ... aos2_frames_set_pose, aos2_extractor_extract_batch_device_async, aos2_frames_build (orders the batch behind the
 *       extraction: the extractor's stream leaves the recording), aos2_frames_search_by_projection_last,
 *       aos2_frames_pose_optimization, ... -- NOTHING runs, the launches are recorded with their arguments
 *   aos2_capture_end(aos2_frames_stream(cur), &g);
 *   per frame: write the image / the pose guess / the local-map rows into the SAME device buffers, aos2_graph_launch(g, stream),
 *   aos2_frames_wait(cur).
 *
 * What is fixed at recording time: every argument passed by value (sizes, thresholds, device addresses).  A count that changes from
 * frame to frame goes through device memory the kernels already read (the frames' keypoint counts d_n, the MapPoint table) or is
 * padded to a capacity: d_local rows of -1 are "no point" (aos2_frames_search_local_points), so n_local can be the capacity of the
 * local map.  Calls that wait on the host (aos2_*_wait, the synchronous forms) cannot be recorded.
 * ------------------------------------------------------------------------------------------ */
typedef struct aos2_graph aos2_graph_t;
/* starts recording on `hip_stream` (a handle's stream, not NULL): the calls that follow enqueue nothing */
int aos2_capture_begin(void *hip_stream);
/* ends the recording (every other stream that joined must have been waited for by `hip_stream`) and builds the replayable graph */
int aos2_capture_end(void *hip_stream, aos2_graph_t **out);
/* enqueues the recorded sequence on `hip_stream` (normally the stream it was recorded on); returns at once */
int aos2_graph_launch(aos2_graph_t *g, void *hip_stream);
int aos2_graph_nodes(const aos2_graph_t *g);   /* kernels + copies of the recording */
void aos2_graph_destroy(aos2_graph_t *g);

/* ------------------------------------------------------------------------------------------
 * Dataset helper (host code; the reference reads its datasets with cv::imread, Examples/RGB-D/rgbd_tum.cc:77-78): the PNG
 * scanline filters undone in place -- rows = h rows of 1 filter byte + stride data bytes as inflated, bpp = bytes per pixel.
 * ------------------------------------------------------------------------------------------ */
int aos2_png_unfilter(uint8_t *rows, int h, int stride, int bpp);

/* ------------------------------------------------------------------------------------------
 * Test taps (no reference equivalent): shared primitives run in isolation.
 * ------------------------------------------------------------------------------------------ */
/* DistributeOctTree (src/ORBextractor.cc:539-763) on the HOST with the routine the device kernel
 * also runs (csrc/octree.h).  Returns the number of kept candidates (indices in out_idx) or <0. */
int aos2_debug_octree_host(const int16_t *xs, const int16_t *ys, const uint8_t *score, int n,
                           int minX, int maxX, int minY, int maxY, int N, int32_t *out_idx, int cap);
/* The extractor's plan for w x h images (level planes, FAST grid cells, slot offsets) as the host computes it; needs no device.
 * levels[nlevels][4] = w, h, pitch, byte offset of the plane in one image's pyramid block; cells[cell_cap][6] = level, vx0, vy0,
 * cw, ch, slot_off (NULL: only *n_cells is returned); totals[2] = pyramid bytes, candidate slots per image.  Fails like an extract
 * call of that size would: AOS2_ERR_TOO_SMALL, AOS2_ERR_ARG. */
int aos2_debug_extractor_plan(const aos2_extractor_t *e, int w, int h, int64_t *levels, int32_t *cells, int cell_cap,
                              int *n_cells, int64_t *totals);
/* rBRIEF steering sin/cos (csrc/sincos_exact.h) evaluated on the host / on the device */
void aos2_debug_sincos_host(float angle_rad, float *s, float *c);
int aos2_debug_sincos_device(const float *angles, int n, float *s, float *c, int device);
/* Every wave / workgroup primitive of csrc/wave_ops.h on caller-supplied per-thread inputs: one workgroup of nt threads (128 or 256,
 * the sizes the library's workgroup scans run with) per case; vi, vd [n_cases][nt]; out_i [n_cases][nt][16] = dpp_u32 and dpp_i32
 * under 0xB1, 0x4E, 0x141, 0x140, row sum, wave sum, wave max, row min, wave min, inclusive scan, block_excl_scan_i32<nt> and its
 * total; out_d [n_cases][nt][7] = dpp_f64 under the four words, row_sum_f64, readlane_f64 of lanes 0 and 63. */
int aos2_debug_wave_ops_device(const int32_t *vi, const double *vd, int n_cases, int nt, int32_t *out_i, double *out_d, int device);
/* row_sums_scatter_f64<K> of csrc/wave_ops.h (K = 7, 36 or 42) run by one wave: v [64][K], a lane's K values; out [64][slots] = every
 * lane's slots afterwards (slots = ceil(K / 16)); owner [K][2] = the lane of a row (0 .. 15) and the slot that row_scatter_owner
 * names for the total of value i. */
int aos2_debug_row_sums_scatter_device(const double *v, int K, double *out, int32_t *owner, int device);
/* aos2_triangulate_matches on the HOST with the routine the device kernels also run (csrc/triangulate.h); needs no device */
int aos2_debug_triangulate_host(const aos2_triang_geom_t *g, int n, const aos2_triang_obs_t *obs1,
                                const aos2_triang_obs_t *obs2, float *x3D, uint8_t *status);
/* aos2_sim3_ransac on the HOST with the routine the device kernels also run (csrc/sim3.h); needs no device.  It stops computing at
 * first_success, where the device reports as if it had. */
int aos2_debug_sim3_host(const aos2_sim3_problem_t *problems, aos2_sim3_result_t *results, int n_problems);
/* aos2_pnp_ransac on the HOST with the routine the device kernels also run (csrc/pnp.h), serially; needs no device.  It stops
 * computing at returned_at and calls Refine() where the loop does, memoised per best set. */
int aos2_debug_pnp_host(const aos2_pnp_problem_t *problems, aos2_pnp_result_t *results, int n_problems);
/* aos2_kfdb_detect / aos2_kfdb_scores on the HOST with the routines the device kernels also run (csrc/kfdb.h), over a literal
 * inverted file (mvInvertedFile: one list of slots per word, in add order), on one core; need no device unless a query's
 * arrays are on the device.  They read and write the same reloc_score as the device calls. */
int aos2_debug_kfdb_host(aos2_kfdb_t *db, const aos2_kfdb_query_t *queries, aos2_kfdb_result_t *results, int nq);
int aos2_debug_kfdb_scores_host(aos2_kfdb_t *db, const aos2_kfdb_query_t *query, const int32_t *slots, int n, float *scores,
                                float *min_score);
/* aos2_vis_count / _count_poses / _motion_costs / _advance on the HOST with the routines the device kernels also run
 * (csrc/visibility.h): the reference's loop, one state and one point at a time on one core, over the handle's map and camera.
 * The same arguments and the same checks; they need no device. */
int aos2_debug_visibility_host(aos2_vis_t *h, int ns, const float *states, int32_t *count, float *sum, uint64_t *mask);
int aos2_debug_visibility_poses_host(aos2_vis_t *h, int ns, const float *T_wb, int32_t *count, float *sum, uint64_t *mask);
int aos2_debug_visibility_motion_costs_host(aos2_vis_t *h, int nm, const int32_t *offsets, const float *states, int thres,
                                            double *cost);
int aos2_debug_visibility_advance_host(aos2_vis_t *h, int ns, const float *states, int thres, int32_t *index);
/* aos2_svc_valid / aos2_svc_motions on the HOST with the routines the device kernels also run (csrc/motion_tw.h): the reference's
 * loops, one motion, one state and one obstacle at a time on one core.  The same arguments and the same checks, made before a
 * device is looked for; they need none. */
int aos2_debug_svc_valid_host(aos2_svc_t *h, int ns, const double *states, uint8_t *valid, uint8_t *collision_free, int32_t *count);
int aos2_debug_svc_motions_host(aos2_svc_t *h, int nm, const double *q1, const double *q2, aos2_svc_motions_out_t *out);
/* aos2_frames_update_local_map / aos2_frames_track_local_map_stats on the HOST, on host arrays: serial, with std::map / std::set
 * keyed by keyframe row the way the reference is written with pointers -- the one-core baseline.  n [batch] = Frame::N, mp
 * [batch][cap] = mvpMapPoints (in / out), outlier [batch][cap]; the other arrays as the device calls take them.  The graph is
 * checked as aos2_local_map_set checks it; no device is needed. */
int aos2_debug_local_map_host(const aos2_local_map_graph_t *g, int batch, int cap, const int32_t *n, int32_t *mp, int32_t *local,
                              int local_cap, int32_t *n_local, int32_t *local_kfs, int kf_cap, int32_t *n_local_kfs, int32_t *ref_kf);
int aos2_debug_local_map_stats_host(const aos2_local_map_graph_t *g, int batch, int cap, const int32_t *n, int32_t *mp,
                                    const uint8_t *outlier, int stereo, int only_tracking, int32_t *stats, int32_t *found_inc);
/* aos2_local_map_keyframe_culling on the HOST with the per-item functions the device kernels also run (csrc/kf_culling.h), in the
 * loop's own order on one core -- the one-core baseline.  The graph and the view are checked as aos2_local_map_set and
 * aos2_local_map_set_culling_view check them, the other arguments as the device call checks them; no device is needed. */
int aos2_debug_keyframe_culling_host(const aos2_local_map_graph_t *g, const aos2_kf_culling_view_t *view, int monocular, int n_cand,
                                     const int32_t *cand, uint8_t *status, int32_t *n_mps, int32_t *n_redundant, int32_t *bad_points,
                                     int bad_cap, int32_t *n_bad_points);
/* aos2_local_map_update_connections on the HOST: the per-item functions the device kernel also runs (csrc/connections.h), in the
 * function's own order on one core -- the one-core baseline and the tap the device is compared with.  The graph is checked as
 * aos2_local_map_set checks it, the other arguments as the device call checks them (the scratch bound aside); no device is needed. */
int aos2_debug_update_connections_host(const aos2_local_map_graph_t *g, int th, int n, const int32_t *kf, const int32_t *n_mp,
                                       const int32_t *mp, int mp_cap, int32_t *n_conn, int32_t *conn_kf, int32_t *conn_w, int conn_cap,
                                       int32_t *n_ordered, int32_t *ordered_kf, int32_t *ordered_w, int ordered_cap);
/* aos2_local_map_update_normal_depth on the HOST: the arithmetic the device kernel also runs (csrc/normal_depth.h), one point and
 * one observation at a time on one core -- the one-core baseline and the tap the device is compared with.  The graph and the view
 * are checked as aos2_local_map_set and aos2_local_map_set_culling_view check them, the other arguments as the device call checks
 * them (the scratch bound aside); no device is needed. */
int aos2_debug_update_normal_depth_host(const aos2_local_map_graph_t *g, const aos2_kf_culling_view_t *view,
                                        const aos2_normal_depth_t *a);
/* aos2_local_map_apply with the rebuild forced onto the HOST, also where the graph is resident: the same checks, the serial
 * restatement on the handle's host copy (refreshed first if it is stale), and the device copy of graph and view marked dirty, so
 * that the next consumer re-uploads everything.  The tap the device rebuild is compared with.  Returns as aos2_local_map_set. */
int aos2_debug_local_map_apply_host(aos2_local_map_t *m, const aos2_local_map_delta_t *d);
/* the math of csrc/motion_tw.h on arrays of n doubles: sin = tw_sin(x), cos = tw_cos(x), atan2 = tw_atan2(y, x), sqrt = sqrt(x),
 * quot = y / x; on the host (device == -1) or in a kernel of one lane per element.  It tells whether a difference between the two
 * sides comes from the math or from the logic.  Any x and y (the domain check of the states does not apply). */
int aos2_debug_tw_math(int device, int n, const double *x, const double *y, double *sin, double *cos, double *atan2, double *sqrt,
                       double *quot);
/* the indices that the draws `row` [min_set] select from 0..n-1 (src/PnPsolver.cc:188-201) as csrc/pnp.h forms them -> indices */
int aos2_debug_pnp_set(int n, const int32_t *row, int min_set, int32_t *indices);
/* the loop of PnPsolver::iterate (:182-239) as csrc/pnp.h replays it over tables: counts [n_iterations] (read from first_iteration),
 * refined [n_iterations] = the inlier count Refine() finds on the set of that iteration, refined_carried that of the carried-in set */
int aos2_debug_pnp_scan(int first_iteration, int n_iterations, const int32_t *counts, const int32_t *refined, int32_t refined_carried,
                        int min_inliers, int best_inliers_in, int32_t *returned_at, int32_t *best_iteration, int32_t *best_inliers);
/* aos2_initializer_initialize on the HOST with the routines the device kernels also run (csrc/initializer.h), serially; needs no
 * device */
int aos2_debug_initializer_host(const aos2_initializer_problem_t *problems, aos2_initializer_result_t *results, int n_problems);
/* cv::SVDecomp(A, w, u, vt, FULL_UV) of a float rows x cols matrix as csrc/initializer.h runs it (16x9, 8x9, 3x3; rows <= 16,
 * cols <= 9, and rows >= cols or rows + 1 == cols).  The Jacobi works on n rows of length m: (n, m) = (cols, rows) for a tall or
 * square matrix (At = A^T), (rows, cols) for a wide one (A itself).  left [n1][m] = the rows after the tail loop (n1 = n, or cols
 * for a wide matrix: its last row is the completion vector), w [n], right [n][n] = the accumulated rotations. */
int aos2_debug_initializer_svd(const float *A, int rows, int cols, float *left, float *w, float *right);
/* the first n values of cv::RNG(0x12345678).next() as csrc/initializer.h generates them */
int aos2_debug_initializer_rng(int n, uint32_t *out);
/* cv::Mat::inv() and cv::determinant of a float 3x3 (row-major) */
int aos2_debug_initializer_inv33(const float *S, float *inv, double *det);
/* aos2_optimize_sim3 on the HOST: the same header (csrc/sim3_opt.h) run serially, edges summed in index order; needs no device */
int aos2_debug_sim3_opt_host(const aos2_sim3_opt_problem_t *p, aos2_sim3_opt_result_t *r, int n_problems);
/* The three steps of csrc/sim3_opt.hip's edge backends alone -- linearise at S_lin, trial at S_trial, reject, in that order, those
 * that `mask` names -- on per-edge state the caller plants: the device form runs SoDevEdges' members in a kernel of sim3_opt_kernel's
 * launch shape and LDS objects (one workgroup per item), the host form SoHostEdges'.  The problem's q12 / t12 / s12 are not read
 * (S_lin and S_trial are given); Huber's delta is formed from th2 as the full call forms it.  act_in / chi_in [2 n + tail] and
 * outlier_in [n + tail] replace the full call's all-ones / zero fill: the `tail` elements behind each array travel with it through the
 * backend's memory and come back behind act / chi / outlier, where a write past the end shows.  A step that is not in `mask` leaves
 * its outputs as the caller passed them.  n_items <= 64, n >= 1; otherwise the argument checks of aos2_optimize_sim3, and a NULL
 * buffer is AOS2_ERR_ARG: reported before anything runs, nothing is written. */
#define AOS2_SIM3_OPT_STEP_LINEARISE 1
#define AOS2_SIM3_OPT_STEP_TRIAL 2
#define AOS2_SIM3_OPT_STEP_REJECT 4
typedef struct {
    aos2_sim3_opt_problem_t problem;
    double S_lin[8], S_trial[8];        /* q (x, y, z, w), t, s */
    const uint8_t *act_in;              /* [2 n + tail]: the edge is in the graph */
    const double *chi_in;               /* [2 n + tail]: the chi2 the edge holds */
    const uint8_t *outlier_in;          /* [n + tail] */
    int32_t tail, remove, mask, pad;
    double *Hb;                         /* linearise: [36] */
    double *pert;                       /* linearise: [28][8], transform k forward at 2 k, inverse at 2 k + 1 */
    double *chi_lin;                    /* linearise: [2 n], chi after it */
    double *trial_sum;                  /* trial: [1] */
    double *chi_trial;                  /* trial: [2 n], chi after it */
    int32_t *flagged;                   /* reject: [1] */
    double *chi;                        /* always: [2 n + tail], chi after the last step */
    uint8_t *act;                       /* always: [2 n + tail] */
    uint8_t *outlier;                   /* always: [n + tail] */
} aos2_sim3_opt_steps_t;
int aos2_debug_sim3_opt_steps_device(aos2_lba_t *s, const aos2_sim3_opt_steps_t *items, int n_items);
int aos2_debug_sim3_opt_steps_host(const aos2_sim3_opt_steps_t *items, int n_items);
/* aos2_optimize_essential_graph on the HOST: the same header (csrc/essential_graph.h) run serially with a skyline LDL^T of the scalar
 * system; n_vertices <= 512 (else AOS2_ERR_CAPACITY); needs no device.  l_blocks is what the device's symbolic phase gives. */
int aos2_debug_essential_graph_host(const aos2_essential_graph_problem_t *p, aos2_essential_graph_result_t *r, int n_problems);
/* pieces of csrc/essential_graph.h on the HOST, n cases: what = 0: Sim3::log, in [n][8] (q x y z w, t, s) -> out [n][7];
 * what = 1: EdgeSim3::computeError log(C * S_v0 * S_v1^-1), in [n][3][8] (C, S_v0, S_v1) -> out [n][7];
 * what = 2: W.lu().solve(t) of a 3x3, in [n][12] (W row-major, t) -> out [n][3] */
int aos2_debug_essential_graph_arith_host(int what, const double *in, int n, double *out);
/* on != 0: later aos2_optimize_essential_graph calls on `s` put HIP events around every launch (slower).  family_ms (may be NULL)
 * receives the device ms of the last such call per kernel family: [0] k_eg_perturb + k_eg_linearise, [1] k_eg_assemble,
 * [2] k_eg_factor_solve, [3] k_eg_begin + k_eg_trial, [4] k_eg_finish (launches that return at once included). */
int aos2_debug_essential_graph_profile(aos2_lba_t *s, int on, float *family_ms);
/* The symbolic phase and k_eg_factor_solve of csrc/essential_graph.hip alone: x = (A + lambda I)^-1 b for the symmetric matrix of
 * n_blocks x n_blocks 7x7 blocks whose lower-triangle blocks are given as triplets (rows[i] > cols[i]; a pair named twice is summed in
 * the order given; val [n_off][49] row-major), diag [n_blocks][49], b and x [7 n_blocks].  *ok = 0: a zero or NaN pivot, x is left
 * as passed in.  *l_blocks = the blocks of L below the diagonal.  1 <= n_blocks <= 8191. */
int aos2_debug_essential_graph_solve_device(aos2_lba_t *s, int n_blocks, int n_off, const int32_t *rows, const int32_t *cols,
                                            const double *val, const double *diag, const double *b, double lambda, double *x,
                                            int32_t *ok, int32_t *l_blocks);
/* The first linearisation of ONE problem as the device forms it: the host phase and the arena layout of aos2_optimize_essential_graph,
 * then k_eg_perturb, k_eg_linearise, k_eg_assemble and k_eg_begin once on the input estimates.  n_vertices <= 512 (else
 * AOS2_ERR_CAPACITY); a problem without a free vertex or without an edge is AOS2_ERR_ARG.  With nf = n_vertices - 1:
 * J [n_edges][2][49] (side 0 / side 1, row-major 7x7; the device buffer is pre-filled with the byte 0x5A, and the Jacobian of a fixed
 * side, which no kernel writes, comes back as that), E [n_edges][7], H [7 nf][7 nf] row-major in hessian order (the free vertices
 * ascending): a diagonal block as stored, a stored block below the diagonal and its transpose, the fill-only blocks of L's pattern
 * included, zero elsewhere; b [7 nf]; chi2 [2] = the control words' lm.currentChi and chi2_initial; *l_blocks as the call reports it. */
int aos2_debug_essential_graph_linearised_device(aos2_lba_t *s, const aos2_essential_graph_problem_t *p, double *J, double *E,
                                                 double *H, double *b, double *chi2, int32_t *l_blocks);
/* One k_eg_trial on ONE problem (limits as above) after the same linearisation (which gives b): x [7 nf] is uploaded as the solver's
 * vector and the control words of an open trial are seeded, running = open = 1, seed_d [3] = lm.lambda, lm.currentChi, lm.ni,
 * seed_i [3] = solved, iterations, qmax (max_iterations = the problem's iterations; the rest as k_eg_begin left it).  est_try and est
 * [n_vertices][8] after the kernel; control_d [6] = lm.lambda, lm.ni, lm.currentChi, lm.iniChi, rho, chi2_initial; control_i [10] =
 * lm.nBad, qmax, open, running, solved, max_iterations, iterations, trials, rejected, accepted_first; sums [2] = the kernel's chi2 of
 * the trial estimates (before a failed solve replaces it by DBL_MAX) and its sum of x (lambda x + b). */
int aos2_debug_essential_graph_trial_device(aos2_lba_t *s, const aos2_essential_graph_problem_t *p, const double *x,
                                            const double *seed_d, const int32_t *seed_i, double *est_try, double *est,
                                            double *control_d, int32_t *control_i, double *sums);
/* aos2_global_bundle_adjustment on the HOST: the same header (csrc/global_ba.h) and the same per-item functions run serially, the
 * reduced system solved by a skyline LDL^T of the scalar system; n_poses <= 2048 (else AOS2_ERR_CAPACITY); needs no device.
 * stop_at_poll as aos2_lba_debug_stop_at_poll.  h_blocks / l_blocks are what the device's symbolic phase gives; ms_device = 0. */
int aos2_debug_global_ba_host(const aos2_lba_problem_t *p, const aos2_gba_options_t *o, aos2_gba_result_t *r, int stop_at_poll);
/* The symbolic phase and k_gba_factor_solve of csrc/global_ba.hip alone: aos2_debug_essential_graph_solve_device for 6x6 blocks
 * (val [n_off][36], diag [n_blocks][36], b and x [6 n_blocks]); 1 <= n_blocks <= 8192. */
int aos2_debug_global_ba_solve_device(aos2_lba_t *s, int n_blocks, int n_off, const int32_t *rows, const int32_t *cols,
                                      const double *val, const double *diag, const double *b, double lambda, double *x,
                                      int32_t *ok, int32_t *l_blocks);
/* The reduced camera system of the FIRST linearisation at `lambda` as the device assembles it (k_gba_linearise, k_gba_sums,
 * k_gba_landmarks, k_gba_assemble): S [6 n_free][6 n_free] row-major, both triangles filled from the stored lower one, with lambda on
 * its diagonal (the Schur complement of H + lambda I), and bs [6 n_free].  n_free = the free keyframes with an edge, 1..512 (else
 * AOS2_ERR_ARG); *h_blocks = its blocks below the diagonal. */
int aos2_debug_global_ba_reduced_device(aos2_lba_t *s, const aos2_lba_problem_t *p, const aos2_gba_options_t *o, double lambda,
                                        int32_t n_free, double *S, double *bs, int32_t *h_blocks);
/* on != 0: later aos2_global_bundle_adjustment calls on `s` put HIP events around every family of launches (slower).  family_ms (may
 * be NULL) receives the device ms of the last such call: [0] k_gba_linearise + k_gba_sums, [1] k_gba_landmarks + k_gba_update,
 * [2] k_gba_assemble, [3] k_gba_factor_solve, [4] k_gba_begin + k_gba_trial_edges + k_gba_decide, [5] k_gba_prepare + k_gba_finish
 * (launches that return at once included). */
int aos2_debug_global_ba_profile(aos2_lba_t *s, int on, float *family_ms);
/* building blocks of the pose solver (csrc/pose_opt.hip) on the device, n independent cases:
 * T_out[i] = exp(upd[i]) * T[i]  (upd: 6 doubles omega | upsilon, T: 7 doubles qx qy qz qw tx ty tz), and
 * x[i] = (H[i] + lambda[i] I)^-1 b[i] with Hb[i] = 21 doubles (upper triangle of H, row by row) + 6 doubles b;
 * ok[i] = 0 where a pivot was not positive (x[i] is left as passed in) */
int aos2_debug_pose_blocks_device(const double *upd, const double *T, double *T_out, const double *Hb, const double *lambda,
                                  double *x, uint8_t *ok, int n, int device);
/* pose_optimization_body of csrc/pose_opt.hip itself, one workgroup per case, in the instantiation the case names:
 * form 0 = <4,256> (n <= 1024), 1 = <8,256> (n <= 2048), 2 = <9,128> (n <= 1152), 3 = <0,256> (edges in global memory, any n).
 * mode 1, edge pass: `pass` once at `pose` with level1 / robust as given -> sums (21 upper-triangle entries of H row by row, 6 of b,
 *         the robust chi2) and chi2 = the stored per-edge chi2 (an edge at level 1: as passed in form 3, 0 in the register forms).
 * mode 2, outlier pass: the reclassification of round `it` once at `pose`, from level1 / robust / outlier / chi2 as given -> the flags
 *         and chi2 as they stand afterwards, n_bad (n_inliers = n - n_bad).
 * mode 0, whole procedure: the body unchanged (the flags and chi2 passed in are ignored) -> outlier, n_bad, n_inliers, pose_out and
 *         Tcw = Converter::toCvMat(pose_out); level1 / robust / chi2 come back as the procedure left them in form 3, as passed otherwise.
 * In modes 1 and 2 pose_out = pose and the LM trials do not run.  AOS2_ERR_ARG (before a device is looked for): a NULL, n_cases < 1,
 * another form or mode, n < 0 or above the form's limit, it outside 0..3. */
typedef struct {
    int32_t n, form, it;
    const float *Xw, *obs, *inv_sigma2;   /* as in aos2_pose_problem_t */
    const uint8_t *stereo;
    float fx, fy, cx, cy, bf;
    double pose[7];                   /* qx qy qz qw tx ty tz */
    uint8_t *level1, *robust, *outlier;   /* [n] in / out */
    double *chi2;                     /* [n] in / out */
    double sums[28];                  /* out (mode 1) */
    double pose_out[7];               /* out */
    float Tcw[16];                    /* out */
    int32_t n_bad, n_inliers;         /* out */
} aos2_pose_pass_case_t;
int aos2_debug_pose_pass_device(aos2_pose_pass_case_t *cases, int n_cases, int mode, int device);
/* The two kernels that solve LocalBA's reduced camera system (csrc/lba.hip: k_ldlt_reg, k_ldlt_dev; this tap and the two below: csrc/lba_taps.hip), alone, with their epilogue: n_cases
 * independent systems H x = bs in ONE launch of each kernel, sized and launched like a Levenberg-Marquardt trial's.  Case c: np[c] free
 * keyframes, n = 6 np[c]; form[c] = 2: k_ldlt_reg (np <= 40), 0: k_ldlt_dev (np <= 154); H: n x n, both triangles (the tap pads it the
 * way the Schur kernel leaves it); the cases' H, bs, b_pose (n each), T (7 per pose: qx qy qz qw tx ty tz) back to back; lambda[c].
 * Out: ok[c] = 1, or 0 on a zero / NaN pivot (255: no kernel touched the case); x = the solution; T_out[i] = exp(x_i) T[i];
 * T_backup = T; scale_terms = x (lambda x + b_pose).  x and scale_terms are in/out: a failed case leaves what the caller passed,
 * T_out = T_backup = T.  AOS2_ERR_ARG (before a device is looked for): a NULL, n_cases < 1, np out of the form's range, another form. */
int aos2_debug_lba_reduced_solve_device(int n_cases, const int32_t *np, const int32_t *form, const double *H, const double *bs,
                                        const double *b_pose, const double *lambda, const double *T, double *x, double *T_out,
                                        double *T_backup, double *scale_terms, uint8_t *ok, int device);

/* The reduced camera system of a LocalBA trial as the shipped kernels assemble it (csrc/lba.hip: k_lin, k_lm_init, k_schur), read before
 * anything solves it.  The host phase is aos2_lba_solve_batch's (csrc/lba_solve.h: build_and_upload), the kernels are enqueued through its
 * helpers (csrc/lba_launch.h), all windows as one group.
 * layout: 0 = slots (k_lin<false> + k_points), 1 = walk (k_lin<true> + k_points_walk) -- as given, whatever the batch size or AOS2_LBA_LAYOUT.
 * stage 0: k_prepare, the start of the first optimisation (residual pass, k_lin with init = 1, k_lm_init), one k_schur.
 * stage 1: the program of aos2_lba_solve_batch for iters_first trials of the first optimisation, k_transition, the start of the second
 *          optimisation, one k_schur.  A window whose first optimisation rejected a step is not there yet: phase, trials_first and
 *          iters_done_first say so (phase 2, trials_first == iters_done_first).
 * lambda: NULL, or one value per window copied into the window's state behind k_lm_init (<= 0: computeLambdaInit's value stays).
 * The stop flags of the problems are ignored.  The caller sizes the arrays of out[w] by the problem: np <= n_poses, nl <= n_points,
 * npad = 6 np rounded up to 16; the tap fills their first np / nl / ... entries.
 * AOS2_ERR_ARG (before a device is looked for): a NULL, n_problems < 1, another layout or stage, iters_first < 1 (iters_second < 1 at
 * stage 1), a window the host phase of the solve refuses, a window without a free keyframe. */
typedef struct {
    int32_t np, nl, npad;             /* out: free keyframes / landmarks with an edge, padded size of Hs */
    int32_t phase;                    /* out: LmState::phase (0 at stage 0, 2 at stage 1) */
    int32_t trials_first, iters_done_first;
    int32_t n_units;                  /* out: k_schur's work units of the window */
    double lambda, current_chi;       /* out: LmState::lambda / currentChi when k_schur ran */
    int32_t *hpose, *hpoint;          /* [np] / [nl]: hidx -> index into the problem's poses / points */
    int32_t *blk_off;                 /* [np (np + 1) / 2 + 1]: first item of every (i1 <= i2) block, upper triangle row by row */
    int32_t *units;                   /* [np + np (np - 1) / 2]: unit codes, kind << 28 | argument (0 DIAG: i; 1 BIG: block rank; 2 PACK: first row) */
    double *pose, *point;             /* [7 n_poses] qx qy qz qw tx ty tz, [3 n_points]: the estimates the system is linearised at */
    uint8_t *e_level1, *e_robust;     /* [n_edges] as the device holds them */
    double *Hpp_init, *b_init;        /* [36 np], [6 np]: Hpp and b_p as the first linearisation (lin_poses_body) left them, before k_schur */
    double *b_p;                      /* [6 np]: b_p as k_schur's DIAG units re-formed it (their Hpp is inside the diagonal blocks of Hs) */
    double *Hll, *b_l;                /* [9 nl], [3 nl] */
    double *Hs, *bs;                  /* [npad x npad] both triangles, tail included; [6 np] */
} aos2_lba_system_t;
int aos2_debug_lba_assemble_device(aos2_lba_t *s, const aos2_lba_problem_t *problems, int n_problems, int layout, int stage,
                                   const double *lambda, aos2_lba_system_t *out);

/* The landmark half of a LocalBA trial and the Levenberg-Marquardt decision, read between the shipped launches (csrc/lba.hip: k_points /
 * k_points_walk with solve = 1 and lm_decide in its last workgroup, k_lin with init = 0, k_transition, k_final).  Host phase, helpers,
 * layout and lambda as in aos2_debug_lba_assemble_device (the two share their preamble, tap_setup of csrc/lba_taps.hip); all windows as one group; aos2_lba_debug_stop_at_poll applies.  Sequence:
 *   k_prepare, the start of the first optimisation, [lambda], trials_before whole trials as the solve enqueues them (k_transition and
 *   the start of the second optimisation before every trial from the iters_first-th on: both are gated by the state),
 *   k_schur + the reduced solve of the trial under test, [scal[3] = 0.0 where force_solver_failed[w]]   -> snapshot 0 (A)
 *   the landmark kernel, solve = 1                                                                      -> snapshot 1 (B)
 *   k_lin, init = 0                                                                                     -> snapshot 2 (C)
 *   tail >= 1: k_transition                                                                             -> snapshot 3 (D)
 *   tail == 2: k_final                                                                                  -> snapshot 4 (E)
 * tail: the k_transition of tail >= 1 does something only where the trial under test ended the first optimisation (xmark); with
 * trials_before >= iters_first the outlier pass has already run in front of a trial and snapshot 3 equals snapshot 2.
 * A snapshot is a stream synchronisation and a copy of the arena; every array of a snapshot whose pointer is not NULL is filled with what
 * the arena holds at that moment (a region no kernel has written yet -- the landmark part of x before the first trial's landmark kernel,
 * the outputs before k_final -- holds what an earlier call left there).
 * force_solver_failed: NULL or one byte per window.  The caller sizes the arrays by the problem (np <= n_poses, nl <= n_points, free-
 * keyframe edges <= n_edges).
 * AOS2_ERR_ARG (before a device is looked for): a NULL, n_problems < 1, another layout or tail, trials_before < 0, iters_first < 1,
 * a window the host phase of the solve refuses, a window without a free keyframe. */
typedef struct {
    double lambda, ni, currentChi, iniChi, final_chi2, final_lambda;
    int32_t phase, run, lin, initp, xmark, it, qmax, nBad;
    int32_t iters_done[2], trials[2];
    int32_t polls, stop_poll, n_active, solver_failed, err_at, ntr;
    double tr_rho[48], tr_temp[48], tr_cur[48], tr_lambda[48];
} aos2_lba_lm_state_t;
typedef struct {
    int32_t taken;                    /* out: the snapshot was made (tail) */
    int32_t pad_;
    aos2_lba_lm_state_t st;           /* out: LmState */
    double scal3;                     /* out: scal[3], 1.0 = the reduced solve succeeded */
    double *est, *bk;                 /* [7 n_poses + 3 n_points]: pose | point, and the push() backup */
    double *x, *b;                    /* [6 np + 3 nl]: pose part, landmark part */
    double *Hll, *Rl, *tmp, *part;    /* [9 nl], [9 np], [6 np], [2 nl] */
    uint8_t *e_level1, *e_robust;     /* [n_edges] */
    double *err, *lrec;               /* [3 n_edges]; [4 n_pl] by position in the landmarks' free-keyframe edge lists */
    uint32_t *erec_flags;             /* [n_edges] by position in the landmarks' edge lists: 1 stereo | 2 robust | 4 level1 */
    float *out_Tcw, *out_xyz;         /* [16 n_poses], [3 n_points] */
    double *out_chi2;                 /* [n_edges] */
    uint8_t *out_outlier;             /* [n_edges] */
} aos2_lba_trial_snap_t;
typedef struct {
    int32_t np, nl, n_pl, n_part;     /* out: free keyframes, landmarks with an edge, free-keyframe edges, workgroups of the landmark kernel */
    int32_t *hpose, *hpoint;          /* [np] / [nl] */
    int32_t *pt_off, *pt_k;           /* [nl + 1], [n_edges]: the landmarks' edge lists (insertion order) */
    int32_t *pl_pos;                  /* [n_edges]: edge -> position of its linearisation record (-1: fixed keyframe) */
    aos2_lba_trial_snap_t snap[5];
} aos2_lba_trial_t;
int aos2_debug_lba_trial_device(aos2_lba_t *s, const aos2_lba_problem_t *problems, int n_problems, int layout, int trials_before,
                                const double *lambda, const uint8_t *force_solver_failed, int tail, aos2_lba_trial_t *out);

#ifdef __cplusplus
}
#endif
#endif /* AOS2_H */
