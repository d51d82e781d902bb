#!/usr/bin/env python
"""Benchmark of the ORB hot path on MI355X (contract: one JSON line on rank 0).

metric    = BASELINE.json's "frames/sec (extract+match+localBA) TUM 640x480".
step      = one pass of the whole per-frame hot path over one batch of B synthetic 640x480 RGB-D frames per GPU, inputs
            resident in HBM before the timed region, every intermediate (keypoints, descriptors, Frame members, matches,
            poses) left in HBM:
              ORBextractor::operator()                                   (extract)
              Frame::Frame: stereo from RGB-D, feature grid
              ORBmatcher::SearchByProjection(CurrentFrame, LastFrame)    (match, Tracking::TrackWithMotionModel)
              Optimizer::PoseOptimization + outlier discard
              Tracking::SearchLocalPoints: isInFrustum + ORBmatcher::SearchByProjection(Frame, local map points)   (match)
              Optimizer::PoseOptimization
            plus, for every `--frames-per-keyframe` (default 8) frames, the keyframe work: Frame::ComputeBoW (ORBVocabulary::transform)
            + ORBmatcher::SearchByBoW(reference keyframe, frame) (Tracking::TrackReferenceKeyFrame's front part, device-resident),
            LocalMapping's matcher calls for it -- ORBmatcher::SearchForTriangulation against its 10 neighbour keyframes
            (CreateNewMapPoints), the search of ORBmatcher::Fuse into each of them and of the scene's local map points into the
            keyframe itself (SearchInNeighbors), device-resident --
            and one Optimizer::LocalBundleAdjustment window of the
            SURVEY section 8(d) size (20 local + 30 fixed keyframes, ~24 k stereo edges), solved by
            aos2_lba_solve_batch concurrently with the tracking chain like the reference's LocalMapping thread
            (host-resident problem arrays: their upload is inside the timed region).
            The B frames of a step are B independent (LastFrame, CurrentFrame) pairs (scenario.py): the reference's chain
            is sequential in time, so a batch is many sequences / replays side by side.
value     = frames/s over all ranks (weak scaling: every rank runs its own batch; no data-path collective).
roofline  = FAST+NMS kernel (the dominant HBM consumer named by north_star): algorithmic bytes P per image
             / kernel time from HIP events on the library's stream.
cpu_baseline = the ORACLE restatement of the SAME composite (oracle/chain.py + oracle LocalBA, C, 1 core) on a bounded sample.

A plain run (`--gpus N --steps K --warmup W`) sets up, warms up, times the K steps and prints the headline line (metric, value,
unit, ms_per_step, dtype, config).  Everything else -- the parity check of the last timed step against the oracle (`parity_checked`),
`cpu_baseline`, `stage_ms`, `roofline*`, `exchange` and the `extra` rows, which take runs of their own -- comes with `--full`.
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (float32 / float64; a fixed sample of the rows of
the larger outputs), so that two builds can be compared output for output on the same generated inputs.
"""
import argparse
import json
import os
import sys
import time

# A step keeps ~12 HIP streams busy (2 pipelines x (extractor + Frame stream + keyframe legs) + 2 LocalBA handles x 2 streams).  The ROCm runtime
# maps the streams of a priority class onto GPU_MAX_HW_QUEUES hardware queues (default 4) by creation order.  Over ~60 runs the queue count
# (4 / 8 / 16) has no effect beyond the line's run-to-run spread, so it is left to the runtime / the caller.

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DUMP_ROWS = 64             # --dump-outputs keeps at most this many rows (frames, keyframe pairs, LocalBA windows) of an output
DUMP_LIMIT = 64 << 20      # bytes of all the files of one --dump-outputs


def dump_rows(n):
    """the rows --dump-outputs keeps of an output with n rows: all of them, or a fixed seeded sample of DUMP_ROWS"""
    if n <= DUMP_ROWS:
        return np.arange(n)
    return np.sort(np.random.default_rng(n).choice(n, DUMP_ROWS, replace=False))


def keypoint_table(kps, n, KP_DTYPE):
    """[B][cap][7] float32 keypoint records (octave / class_id are int32 bit patterns) -> [B][cap][7] float64, zero past n[b]"""
    B, cap = kps.shape[:2]
    rec = np.ascontiguousarray(kps).view(np.uint8).reshape(B, cap, KP_DTYPE.itemsize).copy().view(KP_DTYPE).reshape(B, cap)
    out = np.stack([rec[f].astype(np.float64) for f in KP_DTYPE.names], axis=-1)
    return per_keypoint(out, n)


def per_keypoint(a, n):
    """a [B][cap]... with the entries past n[b] (not written by the step) set to 0"""
    a = np.array(a)
    a[np.arange(a.shape[1])[None, :] >= np.asarray(n).reshape(-1, 1)] = 0
    return a


def dump_outputs(dirname, arrays):
    """--dump-outputs: every array as dirname/<name>.npy, float32 when that holds it exactly (float32, 8- / 16-bit integers), else float64"""
    conv = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        exact32 = a.dtype == np.float32 or (a.dtype.kind in "iub" and a.dtype.itemsize <= 2)
        conv[name] = np.ascontiguousarray(a, dtype=np.float32 if exact32 else np.float64)
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_LIMIT:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes (limit %d)" % (total, DUMP_LIMIT))
    os.makedirs(dirname, exist_ok=True)
    for name, a in conv.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def synth_lba_windows(mix):
    """synth.synth_lba_problems(mix), the job of main()'s helper process"""
    import __graft_entry__ as g
    return g.load_package().synth.synth_lba_problems(mix)


def chain_outputs(pkg, p):
    """what TrackingChain.step() left for its batch: the Frame members a caller reads (keypoints, descriptors, mvuRight / mvDepth,
    mvpMapPoints, mvbOutlier of a fixed sample of frames; N, mTcw and the match / inlier counts of every frame)"""
    F = pkg.capi.Frames
    n = p.d_n.cpu().numpy()
    fr = dump_rows(p.B)
    return {"frame_n": n, "frame_Tcw": p.cur.get(F.TCW), "frame_match_counts": p.d_nm.cpu().numpy(), "frame_sample": fr,
            "frame_keypoints": keypoint_table(p.d_kps.cpu().numpy()[fr], n[fr], pkg.capi.KP_DTYPE),
            "frame_descriptors": per_keypoint(p.d_desc.cpu().numpy()[fr], n[fr]),
            "frame_u_right": per_keypoint(p.cur.get(F.U_RIGHT)[fr], n[fr]), "frame_depth": per_keypoint(p.cur.get(F.DEPTH)[fr], n[fr]),
            "frame_map_points": per_keypoint(p.cur.get(F.MAP_POINTS)[fr], n[fr]), "frame_outlier": per_keypoint(p.cur.get(F.OUTLIER)[fr], n[fr])}


def run_euroc8(args, pkg, torch, dist, rank, world, local_rank, dev, cdev, backend, dist_on):
    """BASELINE configs[4]: EuRoC 752x480 stereo, nfeatures 1200, 8 frames per step sharded over the ranks (strong scaling:
    8 / N frames per rank), every step's slots gathered to rank 0 inside the timed region.  One step of a rank =
    both eyes' ORBextractor::operator() + Frame::ComputeStereoMatches for its frames + pack + gather."""
    cfg = pkg.synth.CONFIGS["euroc"]
    W, H, NF = cfg["w"], cfg["h"], cfg["nfeatures"]
    total = 8
    if total % world:
        raise SystemExit("euroc8: the number of ranks must divide 8")
    B = total // world
    lo = rank * B
    pairs = [pkg.synth.synth_stereo_pair(500 + lo + i, W, H) for i in range(B)]
    d_l = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    d_r = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    xl, xr = pkg.Extractor(nfeatures=NF, device=local_rank), pkg.Extractor(nfeatures=NF, device=local_rank)
    cap = xl.max_keypoints_for(W, H)
    cap = (cap + 3) // 4 * 4
    mk = lambda: (torch.zeros((B, cap, 7), dtype=torch.float32, device=dev), torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev),
                  torch.zeros((B,), dtype=torch.int32, device=dev))
    lk, ld, ln = mk()
    rk, rd, rn = mk()
    ur = torch.zeros((B, cap), dtype=torch.float32, device=dev)
    dp = torch.zeros((B, cap), dtype=torch.float32, device=dev)
    mbf = np.float32(cfg["bf"])
    mb = np.float32(mbf / np.float32(cfg["fx"]))
    sb = pkg.sharding.slot_bytes(cap)
    slot = [torch.zeros((B, sb), dtype=torch.uint8, device=dev) for _ in range(2)]
    bufs = [[torch.empty((B, sb), dtype=torch.uint8, device=cdev) for _ in range(world)] if rank == 0 else None for _ in range(2)]
    work = [None, None]

    def step(s):
        j = s % 2
        if work[j] is not None:
            work[j].wait()
            work[j] = None
        xl.extract_batch_device_async(d_l.data_ptr(), B, W, H, W, W * H, lk.data_ptr(), ld.data_ptr(), cap, ln.data_ptr())
        xr.extract_batch_device_async(d_r.data_ptr(), B, W, H, W, W * H, rk.data_ptr(), rd.data_ptr(), cap, rn.data_ptr())
        pkg.capi.compute_stereo_matches_device(xl, xr, B, lk.data_ptr(), ld.data_ptr(), ln.data_ptr(), rk.data_ptr(), rd.data_ptr(),
                                               rn.data_ptr(), cap, mb, mbf, ur.data_ptr(), dp.data_ptr())
        xl.pack_slots(B, lk.data_ptr(), ld.data_ptr(), ln.data_ptr(), cap, slot[j].data_ptr(), sb, None)   # the null stream
        if dist_on:
            if backend == "nccl":
                work[j] = dist.gather(slot[j], bufs[j], dst=0, async_op=True)
            else:
                work[j] = dist.gather(slot[j].cpu(), bufs[j], dst=0, async_op=True)

    def sync():
        for j in range(2):
            if work[j] is not None:
                work[j].wait()
                work[j] = None
        xl.wait()
        xr.wait()
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        step(i)
    sync()
    import gc
    gc.collect()
    gc.disable()   # (a collection inside a short timed region is a multi-millisecond host pause)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    sync()
    dt = time.perf_counter() - t0
    gc.enable()
    if dist_on:
        t = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:   # rank 0's frames of the last timed step: both eyes' keypoints / descriptors, mvuRight / mvDepth
        hl, hr = ln.cpu().numpy(), rn.cpu().numpy()
        dump_outputs(args.dump_outputs, {
            "left_n": hl, "left_keypoints": keypoint_table(lk.cpu().numpy(), hl, pkg.capi.KP_DTYPE), "left_descriptors": per_keypoint(ld.cpu().numpy(), hl),
            "right_n": hr, "right_keypoints": keypoint_table(rk.cpu().numpy(), hr, pkg.capi.KP_DTYPE), "right_descriptors": per_keypoint(rd.cpu().numpy(), hr),
            "u_right": per_keypoint(ur.cpu().numpy(), hl), "depth": per_keypoint(dp.cpu().numpy(), hl)})
    # ---- parity of the LAST timed step (oracle imported only here): every rank checks its own frames' left keypoints /
    # descriptors and mvuRight / mvDepth, rank 0 also the slots it gathered from every rank, all against the oracle
    parity_checked = None
    if args.verify:
        import __graft_entry__ as g
        g.load_oracle()
        import parity
        bad = []
        hk = lk.cpu().numpy().view(np.uint8).reshape(B, cap, 28).copy().view(pkg.capi.KP_DTYPE).reshape(B, cap)
        hd, hn, hur, hdp = ld.cpu().numpy(), ln.cpu().numpy(), ur.cpu().numpy(), dp.cpu().numpy()
        for i in range(B):
            bad += parity.stereo_slot_mismatches(pkg, hk[i], hd[i], int(hn[i]), hur[i], hdp[i], pairs[i][0], pairs[i][1], cfg,
                                                 tag=f"rank {rank} frame {lo + i}")
        n_slots = 0
        if rank == 0 and dist_on:
            import oracle as O
            got = torch.cat([b_.cpu() for b_ in bufs[(args.steps - 1) % 2]]).numpy()   # [8][slot bytes], rank-major = frame order
            for fr, (k_, d_) in enumerate(pkg.sharding.unpack_slots(got, cap, pkg.capi.KP_DTYPE)):
                okl, odl = O.Extractor(nfeatures=NF).extract(pkg.synth.synth_stereo_pair(500 + fr, W, H)[0])
                n_slots += 1
                if len(k_) != len(okl) or k_.tobytes() != okl.tobytes() or not (d_ == odl).all():
                    bad.append(f"gathered slot of frame {fr}: keypoints / descriptors differ from the oracle's")
        okf = torch.tensor([0 if bad else 1, B, n_slots], dtype=torch.int64, device=cdev)
        if dist_on:
            mn = okf.clone()
            dist.all_reduce(mn, op=dist.ReduceOp.MIN)
            dist.all_reduce(okf, op=dist.ReduceOp.SUM)
            okf[0] = mn[0]
        parity_checked = {"ok": bool(okf[0].item() == 1), "step": "the last timed step", "frames": int(okf[1].item()),
                          "gathered_slots": int(okf[2].item()),
                          "checked": "per frame on its rank: left keypoints, descriptors, mvuRight, mvDepth; on rank 0: keypoints and "
                                     "descriptors of every gathered slot (bit-identical)",
                          "against": "oracle (C restatement; parity unpinned by the reference)", "mismatches_rank0": bad[:10]}
    if rank == 0:
        ok = None
        if dist_on and args.full:
            hdr = torch.stack([b_[:, :4].contiguous().cpu().view(torch.int32).reshape(-1) for b_ in bufs[(args.steps - 1) % 2]])
            ok = bool(((hdr > 0) & (hdr <= cap)).all())
        print(json.dumps({"parity_checked": parity_checked, 
            "metric": "frames/sec (stereo extract + stereo match, 8 frames/step sharded, gathered) EuRoC 752x480",
            "value": total * args.steps / dt, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u8",
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[4]: EuRoC 752x480 stereo, 1200 features, 8 frames per step sharded over the ranks "
                                   "(%d per rank), slots gathered to rank 0 every step" % B,
                       "frames_per_step": total, "frames_per_rank": B, "slot_bytes": sb, "backend": backend, "headers_ok": ok,
                       "stereo_matches_per_frame": float((dp > 0).sum().item()) / B}}))
        if parity_checked is not None and not parity_checked["ok"]:
            sys.stdout.flush()
            raise SystemExit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)   # (0.4 s of timed region: 20 steps = 80 ms left single host hiccups of a few ms visible as +-8 %)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="frames per GPU per step (default: tum 512 -- 512 x 0.95 MB of pyramid = 490 MB: beyond the 256 MiB "
                                                          "Infinity Cache; kitti 256 stereo pairs -- 512 x 1.44 MB)")
    ap.add_argument("--frames-per-keyframe", type=int, default=8, help="one LocalBA window per this many frames")
    ap.add_argument("--workload", default="tum", choices=["tum", "kitti", "euroc8"],
                    help="tum = the BASELINE composite (default); kitti = BASELINE configs[2] + [3]: KITTI 00 stereo 1241x376, 2000 features -- "
                         "both eyes' extraction on two handles, ComputeStereoMatches, the tracking chain, per keyframe ComputeBoW + SearchByBoW "
                         "and one 20-keyframe LocalBA window; euroc8 = BASELINE configs[4]: 8 EuRoC stereo frames per step "
                         "sharded over the ranks (strong scaling), gathered to rank 0 every step")
    ap.add_argument("--lba-mix", default="heterogeneous", choices=["heterogeneous", "homogeneous"],
                    help="LocalBA windows of the timed step: heterogeneous = every window a different problem (10-40 local keyframes, "
                         "2-6 k points, 5-20 %% outliers); homogeneous = round 3's SURVEY 8(d)-size windows (4 distinct, tiled)")
    ap.add_argument("--host-images", action="store_true",
                    help="the reference's host boundary inside the timed step: the images of every step come from page-locked HOST memory "
                         "(ORBextractor::operator() takes a host cv::Mat, src/Frame.cc:276-282) and keypoints / descriptors / mvuRight / mvDepth / "
                         "map point matches / outlier flags / mTcw land in page-locked host arrays, which the parity check then reads; the default "
                         "line reports this form as extra.composite_host_boundary (value stays the HBM-resident form, as BASELINE's contract asks)")
    ap.add_argument("--cpu-frames", type=int, default=0, help="frames for the cpu_baseline sample (0 = auto)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the untimed `extra` rows (matcher / BA / stereo / vocabulary): used for the rocprofv3 summaries, whose per-kernel averages should cover the timed workload only")
    ap.add_argument("--verify", dest="verify", action="store_true", default=None,
                    help="with --full: after the timed region, check results of the LAST timed step against the oracle and report them as "
                         "`parity_checked` (default with --full: on, rank 0, at every N")
    ap.add_argument("--no-verify", dest="verify", action="store_false")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also the parity check against the oracle, cpu_baseline, stage_ms, roofline, exchange and the "
                         "extra rows (other forms of the step, other calls and sizes); without it the run prints the headline figures only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rank 0) as DIR/<name>.npy, float32 / float64, at most 64 MB in all")
    args = ap.parse_args()
    if args.verify and not args.full:
        ap.error("--verify checks the last timed step as part of --full")
    args.verify = args.full and args.verify is not False

    # `python bench.py --gpus N` without a launcher: start the N ranks here (one process per GPU, torch.distributed.run on
    # 127.0.0.1); under a launcher (WORLD_SIZE set) the two must agree -- an 8-GPU line is never printed by one rank
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
                   "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            os.execv(sys.executable, cmd)
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%s ranks" % (args.gpus, os.environ["WORLD_SIZE"]))

    # One helper process, forked here while this process has no thread and no HIP runtime yet: it generates the step's LocalBA windows
    # (seconds of numpy on worker processes of its own) while this process builds the tracking pipelines, which is one core's work.
    helper = None
    if args.workload != "euroc8":
        import multiprocessing
        from concurrent.futures import ProcessPoolExecutor
        helper = ProcessPoolExecutor(1, mp_context=multiprocessing.get_context("fork"))
        helper.submit(os.getpid).result()   # (the worker is forked now, not at the first real job)
    import torch  # first: the library then binds to the same HIP runtime as torch
    import torch.distributed as dist
    import __graft_entry__ as g

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # test hooks (never set by the driver): run the N>1 code path on a box with fewer GPUs
    backend = os.environ.get("AOS2_BENCH_BACKEND", "nccl")
    if os.environ.get("AOS2_BENCH_SHARE_GPU"):
        local_rank = local_rank % torch.cuda.device_count()
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d has no GPU of its own (%d visible); one process per GPU" % (local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # Host placement.  AOS2_BENCH_NUMA=1 binds the process to the CPUs of the GPU's NUMA node (aos2_device_local_cpus) before any handle exists,
    # =setup releases the threads again after the warm-up (handles and page-locked buffers stay on the node), =cores takes one logical CPU per core.
    # Default 0 (the scheduler decides): on the pool's SHARED hosts no mode was consistently better -- pinned to the OTHER socket the step ran at
    # 51-52 k frames/s four times out of four (against 59-63 k), but pinned to the local node it also did so twice on one box where the
    # unpinned runs of the same minutes gave 60 k.  On a dedicated host bind.
    pkg = g.load_package()
    numa_mode = os.environ.get("AOS2_BENCH_NUMA", "0")
    affinity0 = os.sched_getaffinity(0)
    numa_cpus = pkg.bind_to_device_node(local_rank) if numa_mode != "0" else 0
    if numa_mode == "cores" and numa_cpus:   # one logical CPU per core: the lower half of the node's list
        cl = sorted(os.sched_getaffinity(0))
        os.sched_setaffinity(0, cl[: len(cl) // 2])
        numa_cpus = len(cl) // 2
    # the exchange step and the collectives run with more than one rank -- or with ONE rank when AOS2_BENCH_FORCE_DIST=1 (a test
    # hook: the RCCL code path -- process group on the device, gather of device slots on the step's stream, all-reduce, barrier
    # -- on a box with a single GPU; the line then still reports n_gpus = 1)
    dist_on = world > 1 or os.environ.get("AOS2_BENCH_FORCE_DIST") == "1"
    if dist_on:
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    cdev = dev if backend == "nccl" else torch.device("cpu")  # where collective payloads live
    if args.workload == "euroc8":
        run_euroc8(args, pkg, torch, dist, rank, world, local_rank, dev, cdev, backend, dist_on)
        if dist_on:
            dist.barrier()
            dist.destroy_process_group()
        return
    KITTI = args.workload == "kitti"
    cfg_name = "kitti" if KITTI else "tum"
    cfg = pkg.synth.CONFIGS[cfg_name]
    W, H, NF = cfg["w"], cfg["h"], cfg["nfeatures"]
    B = args.batch or (256 if KITTI else 512)
    if KITTI:
        args.no_extra = True   # (the untimed `extra` rows are measured on the TUM workload)

    # ---- scenario: B (LastFrame, CurrentFrame) pairs per step, ALL DISTINCT (no tiling), a different set for every pipeline
    # (step in flight) and every rank, resident in HBM.  AOS2_BENCH_UNIQUE=n tiles n distinct pairs instead (round 3's line: 32).
    import threading
    from concurrent.futures import ThreadPoolExecutor
    NPIPE = max(1, int(os.environ.get("AOS2_BENCH_INFLIGHT", "2")))   # steps in flight (each with its own buffers)
    n_unique = max(1, min(B, int(os.environ.get("AOS2_BENCH_UNIQUE", str(B)))))
    real = None if KITTI else pkg.datasets.dataset_from_env("tum")   # $TUM_FR1_DESK: the recorded frames instead of the generator's
    if real:
        n_unique = min(n_unique, 32)
        pr = pkg.datasets.tum_pairs(real[1], n_unique, step=7 + rank)
        scen = pkg.scenario.tracking_scenario_real(pr, B, cfg="tum")
        scen["dist"] = np.asarray([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)   # Examples/RGB-D/TUM1.yaml
        scens = [scen] * NPIPE
    else:
        scens = [pkg.scenario.tracking_scenario(100 + rank + 1000 * j, B, cfg=cfg_name, n_unique=n_unique, stereo=KITTI) for j in range(NPIPE)]
        scen = scens[0]
    base = scen["cur"]
    fpk = max(1, args.frames_per_keyframe)
    # ---- LocalBA windows of the step: one per frames_per_keyframe frames, every one a DIFFERENT problem drawn over the sizes
    # LocalMapping meets (synth.lba_window_mix: 10-40 local keyframes, 2-6 k points, 4-8 observations per point, 5-20 % gross
    # outliers; src/Optimizer.cc:457-505).  --lba-mix homogeneous = round 3's step: SURVEY 8(d)-size windows, 4 distinct, tiled
    n_win = max(1, B // fpk)
    # AOS2_BENCH_LBA_STEPS_PER_CALL=k: one LocalBA CALL solves the windows of k consecutive steps (all different problems; every step's
    # windows are solved inside the timed region, a step count that is no multiple gets a last call for the rest).  The batch program's cost
    # grows less than linearly with its windows ALONE (64 windows 4.12 ms, 128 7.16, 192 10.5) -- in the composite k = 2 / 3 / 4 gave
    # 70.0, 70.4 / 76.4 / 67.9 k frames/s beside 71.6, 72.6 k for k = 1 in one session (profiles/r06_composite_decomposition.txt): no
    # gain that survives the run-to-run spread, at two to four times the latency of a window's result.  Default 1.
    LBA_SPC = max(1, int(os.environ.get("AOS2_BENCH_LBA_STEPS_PER_CALL", "1")))
    n_win_call = n_win * LBA_SPC
    if KITTI:   # BASELINE configs[3]: the 20-keyframe window of SURVEY 8(d) (20 local + 30 fixed keyframes, ~24 k stereo edges), every one a different problem
        lba_mix = [dict(seed=200000 + 1000 * rank + i, n_local=20, n_fixed=30, n_points=8000) for i in range(n_win_call)]
    elif args.lba_mix == "heterogeneous":
        # One window of the timed, parity-checked step (the last of the batch; AOS2_BENCH_LBA_HARD_EVERY=k: every k-th, 0: none) starts far
        # from the optimum: rejected steps, a continuation round for it alone.  Its end point is gated like every other window's, at the
        # resolution the oracle itself has on it (parity.lba_resolution: the oracle against its own re-associated runs, times parity.LBA_RESOLUTION_FACTOR = 4, never
        # below 1e-5; profiles/r06_lba_sensitivity.txt).  A whole batch with every 8th window like that: extra.local_ba_batch_with_rejected_steps
        lba_mix = pkg.synth.lba_window_mix(rank, n_win_call, hard_every=int(os.environ.get("AOS2_BENCH_LBA_HARD_EVERY", str(n_win))))
    else:
        lba_mix = None
    lba_job = None if lba_mix is None else helper.submit(synth_lba_windows, lba_mix)
    N_LOCAL = 1500
    Chain = pkg.chain.StereoTrackingChain if KITTI else pkg.chain.TrackingChain   # kitti: the stereo Frame constructor (src/Frame.cc:57-113)
    pipes = [Chain(scens[j], device=local_rank, n_local=N_LOCAL) for j in range(NPIPE)]
    # The extractor cuts a batch into chunks on streams of their own so that a chunk's latency-bound octree overlaps the
    # VALU-bound kernels of the others (best for the extractor alone: 3 chunks).  In the composite the other step in flight
    # and the LocalBA batch provide that overlap already, and more streams only contend: measured 53.4 k frames/s with 3
    # chunks, 55.4 k with 1 (AOS2_CHUNKS overrides).
    if "AOS2_CHUNKS" not in os.environ:
        for pp in pipes:
            pp.ex.set_chunks(1)
            if KITTI:
                pp.ex_r.set_chunks(1)
    # the host boundary's uploads run one step ahead (chain.enable_host_boundary(prefetch=True)); AOS2_BENCH_HB_PREFETCH=0: in front of the step
    HB_PREFETCH = os.environ.get("AOS2_BENCH_HB_PREFETCH", "1") != "0"
    if args.host_images:
        for pp in pipes:   # (one step first: the Frame batch's member arrays exist from its first build on)
            pp.step()
            pp.wait()
            pp.enable_host_boundary(prefetch=HB_PREFETCH)
    ex = pipes[0].ex
    cap = pipes[0].cap
    # ---- per keyframe (every `frames_per_keyframe` frames) the front part of Tracking::TrackReferenceKeyFrame (Tracking.cc:858-866):
    # Frame::ComputeBoW (ORBVocabulary::transform, a vocabulary of the ORBvoc shape k = 10, L = 6) + SearchByBoW(reference
    # keyframe, frame), device-resident (chain.ReferenceKeyFrameBoW), on a thread of its own beside the chain
    n_bow = max(1, B // fpk)
    NO_BOW = os.environ.get("AOS2_BENCH_NO_BOW") == "1"   # diagnostics only
    voc_nodes = None if NO_BOW else pkg.synth.synth_vocabulary(400, 10, int(os.environ.get("AOS2_BENCH_VOC_LEVELS", "6")))
    bows = [] if NO_BOW else [pkg.chain.ReferenceKeyFrameBoW(pp, voc_nodes, n_bow) for pp in pipes]
    # ---- and LocalMapping's matcher work for that keyframe (chain.KeyFrameWork, device-resident keyframes): SearchForTriangulation
    # against its nn = 10 best covisible keyframes (CreateNewMapPoints, src/LocalMapping.cc:214-272) and the search part of Fuse of
    # its map points into each of them and of the scene's local map points into the keyframe (SearchInNeighbors, :461-518); on the same
    # side thread as the BoW leg
    # (the neighbour views come from the generator's scenes: with recorded frames the leg is left out and the line says so)
    NO_KFW = NO_BOW or bool(real) or KITTI or os.environ.get("AOS2_BENCH_NO_KEYFRAME_WORK") == "1"
    N_NB = 10
    # SearchInNeighbors also fuses into second-order neighbours (src/LocalMapping.cc:475-485: GetBestCovisibilityKeyFrames(5) of every
    # first-order neighbour, minus those that are first-order targets already -- covisibility lists overlap heavily): 2 new ones per
    # first-order neighbour here = 30 Fuse targets per keyframe (AOS2_BENCH_SECOND_NEIGHBOURS; 0 = round 3's step)
    N_SECOND = max(0, int(os.environ.get("AOS2_BENCH_SECOND_NEIGHBOURS", "2")))
    kfws = [] if NO_KFW else [pkg.chain.KeyFrameWork(pp, voc_nodes, n_bow, n_nb=N_NB, n_second=N_SECOND) for pp in pipes]
    bow_pool = ThreadPoolExecutor(NPIPE)
    bow_jobs = [None] * NPIPE

    def keyframe_job(j):
        t_ = time.perf_counter()
        if bows:
            bows[j].run()
        if kfws:
            kfws[j].run()
        kf_walls.append(time.perf_counter() - t_)
    d_img, d_kps, d_desc, d_n = pipes[0].d_cur, pipes[0].d_kps, pipes[0].d_desc, pipes[0].d_n
    # round 3's windows: the step's LocalBA batch with --lba-mix homogeneous, an extra row of --full (~3 s of generation per window)
    lba_hom_unique, lba_hom = [], []
    if args.full or args.lba_mix == "homogeneous":
        lba_hom_unique = [pkg.synth.synth_lba_problem(10 * rank + i, n_points=8000) for i in range(min(4, n_win))]
        lba_hom = [lba_hom_unique[i % len(lba_hom_unique)] for i in range(n_win_call)]
    if lba_mix is not None:
        lba_unique = lba_job.result()
        lba_probs = lba_unique
    else:
        lba_unique, lba_probs = lba_hom_unique, lba_hom
    helper.shutdown()
    # LocalBA batches in flight (own handle + host thread each): one more than steps in flight -- a call is ~4 ms of host work (structure
    # build, staging) and ~8 ms of device program beside everything else, i.e. two steps long; with two handles the stepping thread
    # waited 6-7 ms of every 8 ms step for it (62.7 k frames/s; three handles 66.7-69.7 k, four 65.9 k, one 51.8 k in one session)
    NLBA = max(1, int(os.environ.get("AOS2_BENCH_LBA_HANDLES", str(NPIPE + 1))))
    lbas = [pkg.LocalBA(device=local_rank) for _ in range(NLBA)]
    # host threads of a handle's per-window work: the node's cores shared among ranks and handles (8 ranks x 2 handles x 32 threads
    # would be 512 threads on 256 cores)
    lba_threads = max(1, min(32, n_win_call, (os.cpu_count() or 1) // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world)) * NLBA)))
    # two handles solve side by side beside the tracking kernels: one program per batch (a handle's two staggered window groups are the
    # faster form only for a batch that has the device to itself: 61 k against 54 k frames/s here; AOS2_BENCH_LBA_GROUPS overrides)
    LBA_GROUPS = int(os.environ.get("AOS2_BENCH_LBA_GROUPS", "1" if NLBA > 1 else "0"))
    for h in lbas:
        h.set_host_threads(lba_threads)
        h.set_window_groups(LBA_GROUPS)
    lba_prep = [h.prepare_batch(lba_probs) for h in lbas]
    pool = ThreadPoolExecutor(NLBA)   # LocalMapping-side threads: one per LocalBA handle (AOS2_BENCH_RUNNER=python)
    lba_jobs = [None] * NLBA
    # The step schedule runs on NATIVE threads by default (csrc/host_runner.cpp): the calls of every job are recorded once
    # (capi.recording()) and replayed -- the Tracking thread's chain on the stepping thread, the keyframe legs and LocalBA on a thread
    # each, like the reference's own std::threads (src/System.cc:136-155).  The five Python threads of earlier rounds handed the
    # interpreter lock to each other between every two C calls: the same steps measured 51.9 / 58.3 / 65.2 k frames/s in three
    # consecutive runs.  AOS2_BENCH_RUNNER=python keeps that form (tests compare the two).
    NATIVE = os.environ.get("AOS2_BENCH_RUNNER", "native") != "python"
    runner = pkg.capi.Runner(NPIPE, NLBA) if NATIVE else None
    if NATIVE:
        runner.set_lba_every(LBA_SPC)
    lba_sched = {"pending": 0, "next": 0, "last": -1}   # (the Python-thread form of the same schedule)
    NO_LBA = os.environ.get("AOS2_BENCH_NO_LBA") == "1"   # diagnostics only: the tracking chains alone (the JSON line is then not the metric)
    # N > 1: the one exchange step of the path -- every step's keypoint / descriptor slots go to
    # rank 0 in one gather (RCCL over xGMI), enqueued behind the step on the step's own stream and left in flight while
    # the next step runs; packed by a device kernel (aos2_extractor_pack_slots)
    sh = pkg.sharding
    sb = sh.slot_bytes(cap)
    gather = None
    if dist_on:
        # the exchange has a stream of its own per pipeline (not the pipeline's: rank 0's next step must not queue behind world - 1
        # incoming slot buffers): the pack kernel is ordered behind the step's extraction on the device (aos2_extractor_pack_slots),
        # the collective behind the pack; the host only makes sure the pack has read the keypoint buffers before the pipeline's
        # next extraction overwrites them (an event two steps old)
        gather = dict(slot=[torch.zeros((B, sb), dtype=torch.uint8, device=dev) for _ in range(NPIPE)], work=[None] * NPIPE,
                      ext=[torch.cuda.Stream(device=dev) for _ in pipes], packed=[None] * NPIPE, t_ev=[None] * NPIPE, us=[],
                      bufs=[[torch.empty((B, sb), dtype=torch.uint8, device=cdev) for _ in range(world)] if rank == 0 else None for _ in range(NPIPE)])

    def gather_step(j):
        p = pipes[j]
        if gather["t_ev"][j] is not None and gather["t_ev"][j][1].query():   # the previous exchange of this pipeline: pack + collective, device time
            gather["us"].append(gather["t_ev"][j][0].elapsed_time(gather["t_ev"][j][1]) * 1e3)
        with torch.cuda.stream(gather["ext"][j]):
            if gather["work"][j] is not None:
                gather["work"][j].wait()   # the STREAM waits for the previous gather of this slot buffer before it is packed again
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            p.ex.pack_slots(B, p.d_kps.data_ptr(), p.d_desc.data_ptr(), p.d_n.data_ptr(), cap, gather["slot"][j].data_ptr(), sb, gather["ext"][j].cuda_stream)
            e0.record()   # (behind the pack's wait for the extraction: what follows is the exchange's own work)
            gather["packed"][j] = torch.cuda.Event()
            gather["packed"][j].record()
            if backend == "nccl":
                gather["work"][j] = dist.gather(gather["slot"][j], gather["bufs"][j], dst=0, async_op=True)
                gather["work"][j].wait()   # (stream-level: orders e1 behind the collective)
                e1.record()
                gather["t_ev"][j] = (e0, e1)
            else:   # gloo (tests): host tensors
                gather["work"][j] = dist.gather(gather["slot"][j].cpu(), gather["bufs"][j], dst=0, async_op=True)

    # where the host thread of the timed steps waits (seconds, summed per kind) and how long the LocalBA calls and keyframe jobs took: the
    # diagnostics behind extra.timed_steps (a few perf_counter reads per step)
    waits = {"local_ba": 0.0, "keyframe_legs": 0.0, "tracking": 0.0}
    lba_walls, kf_walls, step_marks = [], [], []

    def lba_call(jl):
        t_ = time.perf_counter()
        r_ = lbas[jl].solve_prepared(lba_prep[jl])
        lba_walls.append(time.perf_counter() - t_)
        return r_

    job_call_names = {}

    def record_lists():
        """(re-)record the jobs of the native runner from the harness objects as they are now"""
        rec = pkg.capi.recording
        for j_, pp in enumerate(pipes):
            with rec() as c_:
                pp.wait()
            runner.set_list(runner.PIPE_WAIT, j_, c_)
            with rec() as c_:
                pp.step()
                if bows:
                    bows[j_].order()
            runner.set_list(runner.PIPE_STEP, j_, c_)
            with rec() as c_:
                if bows:
                    bows[j_].run_calls()
                if kfws:
                    kfws[j_].run_calls()
            runner.set_list(runner.KF_JOB, j_, c_)
            job_call_names["kf"] = list(c_.names)
        for jl_ in range(NLBA):
            with rec() as c_:
                if not NO_LBA:
                    lbas[jl_].solve_prepared(lba_prep[jl_])
            runner.set_list(runner.LBA_JOB, jl_, c_)

    def step(s):
        if gather is not None and gather["packed"][s % NPIPE] is not None:
            gather["packed"][s % NPIPE].synchronize()   # the last exchange of this pipeline has read its keypoint buffers
        if NATIVE:
            runner.step(s)
            if gather is not None:
                gather_step(s % NPIPE)
            return
        # pipeline s % NPIPE: its previous step (s - NPIPE) is complete before its buffers are reused
        j = s % NPIPE
        p = pipes[j]
        jl = lba_sched["next"]
        lba_now = lba_sched["pending"] + 1 >= LBA_SPC
        t_a = time.perf_counter()
        if lba_now and lba_jobs[jl] is not None:
            lba_jobs[jl].result()
        t_b = time.perf_counter()
        if bow_jobs[j] is not None:
            bow_jobs[j].result()
            bow_jobs[j] = None
        t_c = time.perf_counter()
        p.wait()
        t_d = time.perf_counter()
        waits["local_ba"] += t_b - t_a; waits["keyframe_legs"] += t_c - t_b; waits["tracking"] += t_d - t_c
        step_marks.append(t_d)
        p.step()
        if bows:
            bows[j].order()   # the transform's stream waits for this step's extraction (device side)
        if bows or kfws:
            bow_jobs[j] = bow_pool.submit(keyframe_job, j)
        if gather is not None:
            gather_step(j)
        lba_sched["pending"] += 1
        if lba_now:
            start_lba_py()

    def start_lba_py():
        jl = lba_sched["next"]
        if lba_jobs[jl] is not None:
            lba_jobs[jl].result()
        if not NO_LBA:
            lba_jobs[jl] = pool.submit(lba_call, jl)
        lba_sched.update(pending=0, next=(jl + 1) % NLBA, last=jl)

    def sync():
        if NATIVE:
            runner.sync()
            for j in range(NPIPE):
                if gather is not None and gather["work"][j] is not None:
                    gather["work"][j].wait()
                    gather["work"][j] = None
            torch.cuda.synchronize()
            if dist_on:
                dist.barrier()
            torch.cuda.synchronize()
            return
        if lba_sched["pending"] > 0:
            start_lba_py()
        for jl in range(NLBA):
            if lba_jobs[jl] is not None:
                lba_jobs[jl].result()
                lba_jobs[jl] = None
        for j in range(NPIPE):
            if bow_jobs[j] is not None:
                bow_jobs[j].result()
                bow_jobs[j] = None
            if gather is not None and gather["work"][j] is not None:
                gather["work"][j].wait()
                gather["work"][j] = None
            pipes[j].wait()
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    if os.environ.get("AOS2_BENCH_FAULT"):   # test hook (tests/test_bench_gpu.py): the device table moves, the oracle's inputs do not
        for pp in pipes:
            pp.d_table["pos"][pp.map["mp_last"][0][pp.map["mp_last"][0] >= 0][:40].tolist()] += 0.05
    if NATIVE:
        record_lists()
    for i in range(args.warmup):
        step(i)
    sync()
    if numa_mode == "setup":   # handles, page-locked buffers and threads were created on the node; the threads may roam again
        for t_ in os.listdir("/proc/self/task"):
            try:
                os.sched_setaffinity(int(t_), affinity0)
            except OSError:
                pass
    import gc
    gc.collect()
    gc.disable()   # (a collection inside a short timed region is a multi-millisecond host pause)
    for k_ in waits:
        waits[k_] = 0.0
    del lba_walls[:], kf_walls[:], step_marks[:]
    if NATIVE:
        runner.reset_stats()
    t0 = time.perf_counter()
    if NATIVE and gather is None:
        runner.run(0, args.steps)   # the K steps without a return to the interpreter
    else:
        for i in range(args.steps):
            step(i)
    sync()
    dt = time.perf_counter() - t0
    gc.enable()
    if NATIVE:
        w3 = runner.stats(0)
        waits.update(local_ba=float(w3[0]), keyframe_legs=float(w3[1]), tracking=float(w3[2]))
        lba_walls[:], kf_walls[:], step_marks[:] = list(runner.stats(1)), list(runner.stats(2)), list(runner.stats(3))
    mmm = lambda v: [round(float(x) * 1e3, 3) for x in (min(v), np.median(v), max(v))] if len(v) else None   # noqa: E731
    timed_steps = {"host_thread_waits_ms_per_step": {k_: round(v_ * 1e3 / max(1, args.steps), 3) for k_, v_ in waits.items()},
                   "step_to_step_ms_min_median_max": mmm(np.diff(step_marks)) if len(step_marks) > 2 else None,
                   "local_ba_call_wall_ms_min_median_max": mmm(lba_walls), "keyframe_job_wall_ms_min_median_max": mmm(kf_walls),
                   "keyframe_job_calls_mean_ms": ([[n_, round(float(v_) * 1e3, 3)] for n_, v_ in zip(job_call_names.get("kf", []), runner.stats(100))]
                                                  if NATIVE else None),
                   "note": "the enqueueing thread waits, per step, for the LocalBA call / keyframe job / tracking chain submitted NPIPE steps before; "
                           "a step cannot be shorter than (LocalBA call wall) / (handles in flight)"}
    dt_ranks = [dt]
    if dist_on:
        t = torch.tensor([dt], dtype=torch.float64, device=cdev)
        tl = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(tl, t)
        dt_ranks = [float(x.item()) for x in tl]   # every rank's own clock around its K steps (the line reports the maximum)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    def headline():
        """the result line's figures of the timed steps (rank 0)"""
        _ne = [int(q_["n_edges"]) for q_ in lba_probs]
        if lba_mix is not None:
            lba_desc = ("%d of them starting far from the optimum (rejected steps); " % sum(1 for m_ in lba_mix if "hard" in m_) if any("hard" in m_ for m_ in lba_mix) else "") + \
                       ("%d windows per step, the %d different windows of %d steps solved per call: %d-%d keyframes (%d-%d of them local), %d-%d points, %d-%d edges, mean %.0f edges -- SURVEY 8(d)'s "
                        "window has 24 066" % (n_win, n_win_call, LBA_SPC, min(q_["n_poses"] for q_ in lba_probs), max(q_["n_poses"] for q_ in lba_probs),
                                              min(m_["n_local"] for m_ in lba_mix), max(m_["n_local"] for m_ in lba_mix),
                                              min(q_["n_points"] for q_ in lba_probs), max(q_["n_points"] for q_ in lba_probs), min(_ne), max(_ne), float(np.mean(_ne))))
        else:
            lba_desc = "%d keyframes, %d points, %d edges: SURVEY 8(d); 4 distinct problems tiled" % (lba_probs[0]["n_poses"], lba_probs[0]["n_points"], lba_probs[0]["n_edges"])
        n_kp, nm_host, lba_res = pipes[0].d_n.cpu().numpy(), pipes[0].d_nm.cpu().numpy(), lba_prep[0]["R"]
        return {
            "metric": "stereo frames/sec (extract x2 + stereo match + track + BoW + localBA) KITTI 1241x376" if KITTI else "frames/sec (extract+match+localBA) TUM 640x480",
            "value": world * B * args.steps / dt,
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8 (extract, match) + f64 (PoseOptimization, LocalBA)",
            "data": "real (TUM fr1_desk frames from $TUM_FR1_DESK; LocalBA windows synthetic)" if real else "synthetic",
            "config": {"workload": ("BASELINE configs[2] + [3]: KITTI 00 stereo 1241x376, 2000 features, 8 levels, scale 1.2, FAST 20/7 (Examples/Stereo/KITTI00-02.yaml): "
                                    "per stereo frame both eyes' ORBextractor::operator() on two handles + Frame::ComputeStereoMatches + " if KITTI else
                                    "TUM 640x480 RGB-D, 1000 features, 8 levels, scale 1.2, FAST 20/7: per frame ORBextractor::operator() + ") +
                                   "Frame::Frame + SearchByProjection(Current, Last) + PoseOptimization + SearchLocalPoints(%d local map "
                                   "points) + PoseOptimization; per %d frames one keyframe: Frame::ComputeBoW (vocabulary k = 10, L = 6) + "
                                   "SearchByBoW(reference keyframe, frame), %s"
                                   "and one LocalBundleAdjustment window (%s)" % (N_LOCAL, fpk, ("SearchForTriangulation against %d neighbour keyframes + Fuse (search) into them and %d second-order neighbours + Fuse of the local map points into the keyframe " % (N_NB, N_NB * N_SECOND)) if kfws else "",
                                                            lba_desc),
                       "baseline_metric": "frames/sec (extract+match+localBA) TUM 640\u00d7480, 1/2/4/8 GPU + %HBM roofline",
                       "frames_per_gpu_per_step": B, "frames_per_keyframe": fpk, "local_ba_windows_per_step": n_win,
                       "local_ba_steps_per_call": LBA_SPC, "local_ba_windows_per_call": n_win_call,
                       "local_ba_mix": args.lba_mix, "distinct_frame_pairs_per_step": n_unique, "pipelines": NPIPE,
                       "local_ba_handles_in_flight": NLBA, "step_runner": "native threads (csrc/host_runner.cpp)" if NATIVE else "python threads",
                       "images": ("page-locked host memory every step%s, results to page-locked host arrays (--host-images)" % (", uploaded one step ahead" if HB_PREFETCH else "")) if args.host_images
                                 else "resident in HBM (the host-boundary form: extra.composite_host_boundary)",
                       "hip_hardware_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")), "local_ba_window_groups_per_handle": LBA_GROUPS,
                       "host_cpus_bound_to_the_gpus_numa_node": numa_cpus,
                       "frames_per_s_per_rank": [B * args.steps / d_ for d_ in dt_ranks],
                       "host_threads_per_rank": {"enqueue": 1, "local_ba_handles": NLBA, "local_ba_workers_per_handle": lba_threads,
                                                 "keyframe_legs": NPIPE, "host_cores": os.cpu_count()},
                       "keyframe_legs_per_step": {"reference_keyframe_bow_searches": n_bow if bows else 0,
                                                  "triangulation_pairs": len(kfws[0].tri_pairs) if kfws else 0,
                                                  "fuse_pairs": len(kfws[0].kf1) if kfws else 0,
                                                  "reverse_fuse_problems": n_bow if kfws else 0,
                                                  "note": None if kfws or not real else "the neighbour keyframes are views of the generator's scenes: with recorded "
                                                          "frames the triangulation / fuse leg is left out"},
                       "host_threads": "the GPU path is driven by 1 enqueueing thread + %d LocalMapping-side threads (one per LocalBA handle), each handle "
                                       "building its windows' index structures on up to %d worker threads, + %d threads for the keyframe legs (BoW, triangulation / fuse searches); "
                                       "cpu_baseline is ONE core (the reference's threading per stage)" % (NLBA, lba_threads, NPIPE),
                       "independent_frame_pairs": "the B frames of a step are B independent (LastFrame, CurrentFrame) pairs (%d distinct per pipeline, "
                                                  "another set per pipeline and rank); the chain of ONE sequence is sequential in time and is reported as "
                                                  "extra.tracking_frame_chain_wall_ms" % n_unique,
                       "octree": os.environ.get("AOS2_OCTREE", "device"),
                       "keypoints_per_frame_mean": float(n_kp.mean()),
                       "matches_per_frame_mean": {"search_by_projection_last": float(nm_host[0].mean()), "inliers_1": float(nm_host[1].mean()),
                                                  "search_local_points": float(nm_host[2].mean()), "inliers_2": float(nm_host[3].mean())},
                       "local_ba_iterations": [int(lba_res[0].iters_done_first), int(lba_res[0].iters_done_second)]},
        }

    jv = (args.steps - 1) % NPIPE   # the pipeline of the last timed step: the one the oracle checks (and the cpu_baseline sample runs)
    if args.dump_outputs and rank == 0:   # the last timed step: pipeline jv's frames, its keyframe legs, the windows of the last LocalBA call
        outs = chain_outputs(pkg, pipes[jv])
        if bows:
            kr = dump_rows(n_bow)
            outs.update(keyframe_bow_matches=bows[jv].match[kr], keyframe_bow_nmatches=bows[jv].nmatches)
        if kfws:
            kw = kfws[jv]
            tr, fr, rr = dump_rows(len(kw.match12)), dump_rows(len(kw.best_idx)), dump_rows(len(kw.rev_idx))
            outs.update(triangulation_matches=kw.match12[tr], triangulation_nmatches=kw.nm, fuse_best_idx=kw.best_idx[fr],
                        fuse_best_dist=kw.best_dist[fr], reverse_fuse_best_idx=kw.rev_idx[rr], reverse_fuse_best_dist=kw.rev_dist[rr])
        if not NO_LBA:
            ll = lba_prep[max(0, runner.last_lba() if NATIVE else lba_sched["last"])]
            wr = dump_rows(n_win_call)
            outs.update({"local_ba_" + k_: np.concatenate([ll["arrs"][w][i_].reshape(-1) for w in wr]) for i_, k_ in enumerate(("pose_Tcw", "point_xyz", "edge_outlier"))})
            outs.update(local_ba_final_chi2=[ll["R"][w].final_chi2 for w in wr],
                        local_ba_iterations=[(ll["R"][w].iters_done_first, ll["R"][w].iters_done_second) for w in wr],
                        local_ba_trials=[(ll["R"][w].trials_first, ll["R"][w].trials_second) for w in wr])
        dump_outputs(args.dump_outputs, outs)
    if not args.full:
        if rank == 0:
            print(json.dumps(headline()))
        if dist_on:
            dist.barrier()
            dist.destroy_process_group()
        return
    # ---- the LocalBA device program of the last batch: Levenberg-Marquardt trial slots enqueued for every window against the trials
    # the windows needed (a heterogeneous batch runs in lock step: a window that needs fewer trials leaves its slots empty)
    lock_step = None
    if not NO_LBA:
        jl_ = max(0, runner.last_lba() if NATIVE else lba_sched["last"])   # the handle of the last call
        slots, rounds = lbas[jl_].last_program()
        wslots = lbas[jl_].last_window_slots()
        need = [int(r_.trials_first) + int(r_.trials_second) for r_ in lba_prep[jl_]["R"]]
        edges = [int(q_["n_edges"]) for q_ in lba_probs]
        lock_step = {"trial_slots_enqueued": slots, "host_rounds": rounds, "windows": n_win_call, "window_slots": wslots,
                     "trials_needed_min_mean_max": [min(need), float(np.mean(need)), max(need)],
                     "windows_with_rejected_or_skipped_trials": int(sum(1 for n_ in need if n_ != 15)),
                     "slots_over_trials": wslots / max(1, sum(need)),
                     "largest_window_edges_over_mean": max(edges) / (sum(edges) / len(edges)),
                     "note": "the first round of the program holds as many trials as there are iterations (5 + 10) for every window; a window "
                             "that is not finished then (rejected steps) gets a continuation round with the other unfinished windows only, "
                             "compacted, sized for what it still needs.  slots_over_trials = trial slots summed over the windows each round "
                             "covered / trials the windows needed (1.0 = no launch covered a window with nothing left to do; a window whose "
                             "optimisation ends early leaves its remaining slots of the round empty)"}
    scen_v = scens[jv]
    # ---- what the LAST timed step left behind, copied before anything else reuses the buffers: checked against the oracle
    # below (`parity_checked`).  The oracle is only imported here, after the timed region.
    do_verify = args.verify   # rank 0, at every N
    snap = None
    if rank == 0 and do_verify:
        g.load_oracle()
        import parity
        lp, ll = pipes[jv], lba_prep[max(0, runner.last_lba() if NATIVE else lba_sched["last"])]
        lb = bows[jv] if bows else None
        snap = dict(chain=parity.chain_snapshot_host(pkg, lp) if args.host_images else parity.chain_snapshot(pkg, lp), pipe=lp, bow=None if lb is None else lb.get_results(),
                    kfw=kfws[jv].snapshot() if kfws else None,
                    lba=[] if NO_LBA else [pkg.LocalBA._result(ll["R"][w], tuple(a.copy() for a in ll["arrs"][w])) for w in range(n_win_call)])
    # ---- the same steps without the keyframe legs: the composite as round 2 measured it, and with the BoW leg only (comparability)
    dt_nobow = dt_bowonly = dt_hom = None
    if bows and os.environ.get("AOS2_BENCH_SKIP_R02_FORM") != "1":
        def short_run(n2):
            if NATIVE:
                record_lists()   # (the harness objects changed: the jobs are recorded again)
            for i in range(2):
                step(i)
            sync()
            t0 = time.perf_counter()
            for i in range(n2):
                step(i)
            sync()
            return (time.perf_counter() - t0) / n2
        saved, saved_kfw, n2 = list(bows), list(kfws), max(10, min(args.steps, 50))
        if lba_mix is not None and not NO_LBA and not KITTI:   # the same steps with round 3's LocalBA windows (SURVEY 8(d) size, 4 distinct, tiled)
            saved_prep = list(lba_prep)
            lba_prep[:] = [h.prepare_batch(lba_hom) for h in lbas]
            dt_hom = short_run(n2)
            lba_prep[:] = saved_prep
        if kfws:
            kfws.clear()
            dt_bowonly = short_run(n2)
        bows.clear()
        dt_nobow = short_run(n2)
        bows.extend(saved)
        kfws.extend(saved_kfw)
        if NATIVE:
            record_lists()
    # ---- the same steps with the reference's HOST boundary (--host-images): images up from page-locked memory, the Frame's members
    # down into page-locked arrays, every step; checked against the oracle from those host arrays (below)
    hb_run = None
    if not args.host_images and not args.no_extra and not NO_LBA and os.environ.get("AOS2_BENCH_SKIP_HOST_BOUNDARY") != "1":
        for pp in pipes:
            pp.enable_host_boundary(prefetch=HB_PREFETCH)
        if NATIVE:
            record_lists()
        n2 = max(10, min(args.steps, 50))
        while (n2 - 1) % NPIPE != jv:   # (its last step on the pipeline whose oracle results the check below holds)
            n2 += 1
        for i in range(2):
            step(i)
        sync()
        t0 = time.perf_counter()
        for i in range(n2):
            step(i)
        sync()
        dt_hb = (time.perf_counter() - t0) / n2
        jh = (n2 - 1) % NPIPE
        hb_run = dict(dt=dt_hb, scen=scens[jh], up=pipes[jh].hb["up_bytes"], down=pipes[jh].hb["down_bytes"],
                      snap=parity.chain_snapshot_host(pkg, pipes[jh]) if snap is not None else None)
        for pp in pipes:
            pp.enable_host_boundary(False)
        if NATIVE:
            record_lists()
    # ---- a LocalBA batch whose windows need DIFFERENT numbers of trials (every 8th window starts far from the optimum: rejected steps,
    # optimisations that end early), alone on the device: the program's rounds, the lock-step ratio, the decisions against the oracle
    lba_hard = None
    if rank == 0 and world == 1 and not args.no_extra and not NO_LBA and not KITTI and args.lba_mix == "heterogeneous":
        hm = pkg.synth.lba_window_mix(rank, n_win, hard_every=8)
        hp = pkg.synth.synth_lba_problems(hm)
        hprep = lbas[0].prepare_batch(hp)
        lbas[0].set_window_groups(0)
        lbas[0].solve_prepared(hprep)
        tms = []
        for _ in range(3):
            torch.cuda.synchronize()
            ta = time.perf_counter()
            lbas[0].solve_prepared(hprep)
            tms.append((time.perf_counter() - ta) * 1e3)
        lbas[0].set_window_groups(LBA_GROUPS)
        hneed = [int(r_.trials_first) + int(r_.trials_second) for r_ in hprep["R"]]
        lba_hard = dict(mix=hm, probs=hp, res=[pkg.LocalBA._result(hprep["R"][w], tuple(a.copy() for a in hprep["arrs"][w])) for w in range(n_win)],
                        row={"windows": n_win, "windows_started_off_the_optimum": sum(1 for m_ in hm if "hard" in m_),
                             "call_wall_ms_median": float(np.median(tms)), "device_ms": float(hprep["R"][0].ms_device),
                             "trial_slots_enqueued": lbas[0].last_program()[0], "host_rounds": lbas[0].last_program()[1],
                             "trials_needed_min_mean_max": [min(hneed), float(np.mean(hneed)), max(hneed)],
                             "windows_not_needing_15_trials": int(sum(1 for n_ in hneed if n_ != 15)),
                             "slots_over_trials": lbas[0].last_window_slots() / max(1, sum(hneed))})
    # ---- stage times of one synchronous pass (every stage waited for: wall clock incl. launch latency)
    def timed(fn):
        torch.cuda.synchronize()
        ta = time.perf_counter()
        fn()
        return (time.perf_counter() - ta) * 1e3
    p0, sc = pipes[0], scen
    W_, H_ = W, H
    composite_stage = {}
    if KITTI:
        def _one_eye():
            p0.ex.extract_batch_device_async(p0.d_cur.data_ptr(), B, W_, H_, W_, W_ * H_, p0.d_kps.data_ptr(), p0.d_desc.data_ptr(), cap, p0.d_n.data_ptr())
            p0.ex.wait()
        composite_stage["extract_left_eye_alone"] = timed(_one_eye)
    def _extract():   # (kitti: both eyes on their handles + ComputeStereoMatches behind them)
        p0.enqueue_extract()
        p0.wait_extract()
    composite_stage["extract_both_eyes_and_stereo_matches" if KITTI else "extract"] = timed(_extract)
    def _build():
        p0.enqueue_build()
        p0.cur.set_pose(p0.d_guess.data_ptr())
        p0.cur.wait()
    composite_stage["frame_build"] = timed(_build)
    def _w(fn):
        def g_():
            fn()
            p0.cur.wait()
        return g_
    composite_stage["search_by_projection_last"] = timed(_w(lambda: p0.cur.SearchByProjectionLast(p0.last, p0.table, p0.th_last, False, True, p0.d_nm[0].data_ptr())))
    composite_stage["pose_optimization_1"] = timed(_w(lambda: (p0.cur.PoseOptimization(p0.table, p0.d_nm[1].data_ptr()), p0.cur.discard_outliers())))
    composite_stage["search_local_points"] = timed(_w(lambda: p0.cur.SearchLocalPoints(p0.table, p0.d_local.data_ptr(), N_LOCAL, p0.th_local, p0.nnratio_local, p0.d_nm[2].data_ptr())))
    composite_stage["pose_optimization_2"] = timed(_w(lambda: p0.cur.PoseOptimization(p0.table, p0.d_nm[3].data_ptr())))
    if bows:
        def _bow():
            bows[0].order()
            bows[0].run()
        composite_stage["reference_keyframe_bow_wall"] = timed(_bow)
        composite_stage["reference_keyframe_bow_device"] = {"transform": bows[0].last_ms[0], "search_by_bow": bows[0].last_ms[1], "frames": n_bow}
    if kfws:
        composite_stage["keyframe_work_wall"] = timed(lambda: kfws[0].run(timed=True))
        composite_stage["keyframe_work_calls"] = {"search_for_triangulation": kfws[0].last_ms[0], "fuse": kfws[0].last_ms[1],
                                                  "fuse_pairs": len(kfws[0].kf1), "triangulation_pairs": len(kfws[0].tri_pairs), "keyframes": n_bow,
                                                  "neighbours": N_NB, "second_order_fuse_targets_per_neighbour": N_SECOND}
    composite_stage["local_ba_batch_wall"] = timed(lambda: lbas[0].solve_prepared(lba_prep[0]))
    composite_stage["local_ba_batch_device"] = float(lba_prep[0]["R"][0].ms_device)
    composite_stage["note"] = ("one synchronous pass, every stage waited for (wall clock incl. launch latency); the timed steps enqueue "
                               "the tracking stages back to back, keep two steps in flight and overlap the LocalBA batch")

    # ---- ORBextractor-only throughput (BASELINE configs[1]), K steps in flight, each with its own output buffers
    nbuf = 3
    xk = [torch.empty((B, cap, 7), dtype=torch.float32, device=dev) for _ in range(nbuf)]
    xd = [torch.empty((B, cap, 32), dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    xn = [torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(nbuf)]

    def step_sync():
        ex.extract_batch_device(d_img.data_ptr(), B, W, H, W, W * H, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr())

    def xsync():
        ex.wait()
        torch.cuda.synchronize()

    xsync()
    t1 = time.perf_counter()
    for i in range(args.steps):
        if i >= nbuf:
            pass   # (stream order: chunk c of step i runs behind chunk c of step i - nbuf on the same stream)
        j = i % nbuf
        ex.extract_batch_device_async(d_img.data_ptr(), B, W, H, W, W * H, xk[j].data_ptr(), xd[j].data_ptr(), cap, xn[j].data_ptr())
        if i % nbuf == nbuf - 1:
            ex.wait()   # the buffers of a batch are not reused while it is in flight (include/aos2.h)
    xsync()
    dt_extract = time.perf_counter() - t1
    t1 = time.perf_counter()
    for _ in range(args.steps):
        step_sync()
    xsync()
    dt_sync = time.perf_counter() - t1
    # per-stage device times of one un-chunked (single-stream) pass; `value` above is measured with the
    # default multi-stream chunking
    ex.set_chunks(1)
    step_sync()
    stage = ex.last_timing()
    ex.set_chunks(int(os.environ.get("AOS2_CHUNKS", "0")))
    fast_ms = ex.bench_fast(20)

    n_kp = d_n.cpu().numpy()
    gather_ok = None
    if dist_on and rank == 0:   # the slots gathered in the last step carry every rank's keypoint counts
        hdr = torch.stack([b_[:, :4].contiguous().cpu().view(torch.int32).reshape(-1) for b_ in gather["bufs"][(args.steps - 1) % NPIPE]])
        gather_ok = bool(((hdr > 0) & (hdr <= cap)).all())
        assert gather_ok, "gathered slot headers corrupt"

    # secondary measurements of the other hot-path rows (reported, not part of `value`)
    extra = {"local_ba_lock_step": lock_step, "timed_steps": timed_steps,
             "composite_with_homogeneous_local_ba_windows": None if dt_hom is None else {
                 "note": "the timed steps with round 3's LocalBA batch instead: %d windows of the SURVEY 8(d) size (%d keyframes, %d points, "
                         "%d edges), 4 distinct problems tiled" % (n_win, lba_hom[0]["n_poses"], lba_hom[0]["n_points"], lba_hom[0]["n_edges"]),
                 "frames_per_s": world * B / dt_hom, "ms_per_step": dt_hom * 1e3},
             "local_ba_batch_with_rejected_steps": None if lba_hard is None else lba_hard["row"],
             "composite_host_boundary": None if hb_run is None else {
                 "note": "the timed steps with the reference's HOST boundary (bench.py --host-images makes it the timed form): every step's %d images "
                         "arrive from page-locked host memory (ORBextractor::operator() takes a host cv::Mat, src/Frame.cc:276-282) and mvKeys / "
                         "mDescriptors / N / mvuRight / mvDepth / mvpMapPoints / mvbOutlier / mTcw / the match counts of every frame land in page-locked "
                         "host arrays; `value` above is the HBM-resident form BASELINE's contract asks for.  " % B +
                         ("The images of a step are copied up during the pipeline's previous step into a staging buffer on the device (a frame "
                          "grabber's double buffer) and moved into place by a device-to-device copy when the step starts; AOS2_BENCH_HB_PREFETCH=0 "
                          "puts the upload in front of the step: 44-52 k frames/s" if HB_PREFETCH else "uploads in front of every step (AOS2_BENCH_HB_PREFETCH=0)"),
                 "uploads_one_step_ahead": HB_PREFETCH,
                 "frames_per_s": world * B / hb_run["dt"], "ms_per_step": hb_run["dt"] * 1e3,
                 "host_to_device_MB_per_step": hb_run["up"] / 1e6, "device_to_host_MB_per_step": hb_run["down"] / 1e6,
                 "pcie_GB_per_s": (hb_run["up"] + hb_run["down"]) / hb_run["dt"] / 1e9,
                 "parity_checked_from_host_arrays": None},
             "composite_without_reference_keyframe_bow": None if dt_nobow is None else {
                 "note": "the timed steps without the per-keyframe legs (ComputeBoW + SearchByBoW, SearchForTriangulation + Fuse) = the "
                         "composite of round 2's bench line",
                 "frames_per_s": world * B / dt_nobow, "ms_per_step": dt_nobow * 1e3},
             "composite_with_the_bow_leg_only": None if dt_bowonly is None else {
                 "note": "the timed steps with ComputeBoW + SearchByBoW per keyframe but without SearchForTriangulation + Fuse",
                 "frames_per_s": world * B / dt_bowonly, "ms_per_step": dt_bowonly * 1e3},
             "extract_only": {
        "note": "BASELINE configs[1]: ORBextractor::operator() alone over the same frames (round 1's headline)",
        "frames_per_s_async": world * B * args.steps / dt_extract, "ms_per_step_async": dt_extract / args.steps * 1e3,
        "frames_per_s_synchronous_call": world * B * args.steps / dt_sync, "ms_per_step_synchronous_call": dt_sync / args.steps * 1e3,
        "async_note": "aos2_extractor_extract_batch_device_async, %d rotating output buffer sets, one wait per %d steps" % (nbuf, nbuf)}}
    if rank == 0 and world == 1 and not args.no_extra:   # (N = 1 only: the other ranks would wait at the final barrier)
        try:
            S = pkg.synth
            rng = np.random.default_rng(0)
            m = pkg.Matcher(0.7, True, device=local_rank)
            nq = nt = 2000
            dq = torch.from_numpy(S.synth_descriptors(rng, nq)).to(dev)
            dt_ = torch.from_numpy(S.synth_descriptors(rng, nt)).to(dev)
            o1, o2, o3 = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(3))
            m.hamming_best2_device(dq.data_ptr(), nq, dt_.data_ptr(), nt, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), 5)
            hms = m.hamming_best2_device(dq.data_ptr(), nq, dt_.data_ptr(), nt, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), 50)
            extra["hamming_2000x2000_ms"] = hms
            extra["hamming_pair_distances_per_s"] = nq * nt / (hms * 1e-3)
            probs = [S.synth_bow_problem(100 + i, 1000, 1000, nnratio=0.7) for i in range(64)]
            m.SearchByBoW(probs)
            tb = time.perf_counter()
            m.SearchByBoW(probs)
            extra["search_by_bow_64pairs_wall_ms"] = (time.perf_counter() - tb) * 1e3
            extra["search_by_bow_64pairs_device_ms"] = m.last_device_ms()
            f, mp = S.synth_proj_mp_problem(0)
            m2 = pkg.Matcher(0.8, True, device=local_rank)
            m2.SearchByProjection(f, mp, th=3.0)
            tb = time.perf_counter()
            m2.SearchByProjection(f, mp, th=3.0)
            extra["search_by_projection_1500mp_wall_ms"] = (time.perf_counter() - tb) * 1e3
            extra["search_by_projection_1500mp_device_ms"] = m2.last_device_ms()
            # the per-frame tracking chain of the reference (Tracking::TrackWithMotionModel, Tracking.cc:862-870): one frame
            # at a time through the host-pointer calls -- operator(), SearchByProjection(Cur, Last), PoseOptimization --
            # wall time of each call as a caller sees it (ctypes wrapper included), median of 20
            ex1 = pkg.Extractor(nfeatures=NF, device=local_rank)
            img1 = np.ascontiguousarray(base[0])
            cur_l, pl_l = S.synth_proj_last_problem(5, n=1000)
            m3 = pkg.Matcher(0.9, True, device=local_rank)
            pp1 = S.synth_pose_problem(9, n=800)
            ba1 = pkg.LocalBA(device=local_rank)
            chain = {"extract": [], "search_by_projection_last": [], "pose_optimization": []}
            for it_ in range(23):
                t0_ = time.perf_counter(); ex1(img1)
                t1_ = time.perf_counter(); m3.SearchByProjectionLast(cur_l, pl_l, float(pl_l["th"]), int(pl_l["mono"]))
                t2_ = time.perf_counter(); ba1.PoseOptimization(pp1)
                t3_ = time.perf_counter()
                if it_ >= 3:
                    chain["extract"].append(t1_ - t0_); chain["search_by_projection_last"].append(t2_ - t1_)
                    chain["pose_optimization"].append(t3_ - t2_)
            tf = {k: float(np.median(v)) * 1e3 for k, v in chain.items()}
            tf["total_ms"] = sum(tf.values())
            tf["note"] = "single 640x480 frame, 1000 features, 1000 last-frame points, 800 pose correspondences; host buffers in and out"
            extra["tracking_frame_chain_wall_ms"] = tf
            # ONE sequence, one frame at a time, device-resident (the reference's real calling pattern, Tracking::Track /
            # Examples/RGB-D/rgbd_tum.cc:91-108): the whole chain of a frame enqueued and waited for, median of 40
            sc1 = pkg.scenario.tracking_scenario(5, 1, n_unique=1)
            tc1 = pkg.chain.TrackingChain(sc1, device=local_rank, n_local=N_LOCAL)
            lat = []
            for it_ in range(45):
                torch.cuda.synchronize()
                ta_ = time.perf_counter()
                tc1.step()
                tc1.wait()
                lat.append(time.perf_counter() - ta_)
            ms1 = float(np.median(lat[5:])) * 1e3
            # ... the same calls recorded once and replayed with ONE launch per frame (include/aos2.h "Replay of a fixed call sequence"):
            # the members the replay leaves are compared with the plain calls' (bytes)
            tc1.wait()
            F1 = pkg.capi.Frames
            plain_members = [tc1.cur.get(F1.TCW).tobytes(), tc1.cur.get(F1.MAP_POINTS).tobytes(), tc1.cur.get(F1.OUTLIER).tobytes(),
                             tc1.d_nm.cpu().numpy().tobytes(), tc1.d_desc.cpu().numpy().tobytes()]
            gr1 = tc1.capture_step()
            tc1.d_nm.zero_(); tc1.d_desc.zero_()
            lat = []
            for it_ in range(45):
                torch.cuda.synchronize()
                ta_ = time.perf_counter()
                tc1.step_graph()
                tc1.cur.wait()
                lat.append(time.perf_counter() - ta_)
            ms1g = float(np.median(lat[5:])) * 1e3
            replay_members = [tc1.cur.get(F1.TCW).tobytes(), tc1.cur.get(F1.MAP_POINTS).tobytes(), tc1.cur.get(F1.OUTLIER).tobytes(),
                              tc1.d_nm.cpu().numpy().tobytes(), tc1.d_desc.cpu().numpy().tobytes()]
            replay = {"ms_per_frame": ms1g, "frames_per_s": 1e3 / ms1g, "launches_recorded": gr1.nodes(),
                      "same_members_as_the_plain_calls": replay_members == plain_members,
                      "note": "aos2_capture_begin / the calls of the frame / aos2_capture_end once, then aos2_graph_launch + aos2_frames_wait per "
                              "frame: the kernels run back to back instead of ~6 us apart"}
            gr1.close()
            # ... and with the next image's ExtractORB enqueued beside the frame's tracking (chain.step_pipelined): wall clock of 200 frames
            tc1.wait()
            for it_ in range(10):
                tc1.step_pipelined(); tc1.wait_frame()
            ta_ = time.perf_counter()
            for it_ in range(200):
                tc1.step_pipelined(); tc1.wait_frame()
            ms1p = (time.perf_counter() - ta_) * 1e3 / 200
            tc1.wait()
            extra["single_sequence"] = {"ms_per_frame": ms1, "frames_per_s": 1e3 / ms1, "recorded_sequence_replayed": replay,
                                        "next_image_extracted_beside_tracking": {"ms_per_frame": ms1p, "frames_per_s": 1e3 / ms1p,
                                            "note": "the same chain, every frame waited for before the next one's Frame::Frame, but the NEXT image's "
                                                    "operator() is enqueued on the extractor's stream while this frame is tracked (it depends on the image "
                                                    "alone, Tracking.cc:207-235): period = max(extraction, tracking); a frame's latency is ms_per_frame above"},
                                        "note": "B = 1, device-resident chain: operator() + Frame::Frame + SearchByProjection(Current, Last) + "
                                                "PoseOptimization + SearchLocalPoints + PoseOptimization, enqueue + wait per frame (latency-bound: "
                                                "dependent single-workgroup kernels -- PoseOptimization, the level-0 octree, the greedy resolves)"}
            del tc1
            pb = [S.synth_proj_mp_problem(700 + i) for i in range(64)]
            m2.SearchByProjectionBatch([q[0] for q in pb], [q[1] for q in pb], th=3.0)
            m2.SearchByProjectionBatch([q[0] for q in pb], [q[1] for q in pb], th=3.0)
            extra["search_by_projection_64frames_1500mp_device_ms"] = m2.last_device_ms()
            prob = S.synth_lba_problem(0)
            ba = pkg.LocalBA(device=local_rank)
            ba.LocalBundleAdjustment(prob)
            tb = time.perf_counter()
            r = ba.LocalBundleAdjustment(prob)
            lba_wall = (time.perf_counter() - tb) * 1e3
            pps = [S.synth_pose_problem(200 + i, n=800) for i in range(64)]
            ba.PoseOptimization(pps)
            tb = time.perf_counter()
            ba.PoseOptimization(pps)
            extra["pose_optimization_64frames_800pts"] = {"wall_ms": (time.perf_counter() - tb) * 1e3,
                                                          "device_ms": ba.pose_last_device_ms()}
            ba.PoseOptimization(pps[0])
            extra["pose_optimization_1frame_device_ms"] = ba.pose_last_device_ms()
            extra["local_ba"] = {"edges": prob["n_edges"], "keyframes": prob["n_poses"], "points": prob["n_points"],
                                 "wall_ms": lba_wall, "device_ms": r["ms_device"],
                                 "iterations": r["iters"], "trials": r["trials"],
                                 "bound": "latency (4 dependent launches per Levenberg-Marquardt trial, the whole solve enqueued at once; half of a trial is the serial pivot chain of the reduced-system LDL^T)"}
            # independent windows (several maps / offline windows, SURVEY 8(e): LocalBA = replicas only): one handle
            # and one host thread per window; the latency-bound kernels of the windows overlap on the GPU
            import threading
            nwin = 8
            bas = [pkg.LocalBA(device=local_rank) for _ in range(nwin)]
            probs_w = [S.synth_lba_problem(i) for i in range(nwin)]
            for b_, q_ in zip(bas, probs_w):
                b_.LocalBundleAdjustment(q_)
            wall_w = 1e9
            for _rep in range(3):   # best of 3 (the first concurrent round also pays thread start-up)
                ths = [threading.Thread(target=b_.LocalBundleAdjustment, args=(q_,)) for b_, q_ in zip(bas, probs_w)]
                tb = time.perf_counter()
                [t_.start() for t_ in ths]
                [t_.join() for t_ in ths]
                wall_w = min(wall_w, (time.perf_counter() - tb) * 1e3)
            extra["local_ba"]["concurrent_windows"] = {"windows": nwin, "wall_ms": wall_w, "windows_per_s": nwin / wall_w * 1e3}
            # stereo front-end on the bench frames themselves (same launch shapes as the timed steps, so the
            # rocprofv3 averages of the extractor kernels stay comparable): right eye = left eye shifted by a
            # per-row-band disparity + noise; both eyes' operator() + Frame::ComputeStereoMatches, device-resident
            srng = np.random.default_rng(77)
            rbase = np.empty_like(base)
            for u in range(n_unique):
                for y0 in range(0, H, 32):
                    dsp = int(srng.integers(4, 40))
                    rows = base[u, y0:y0 + 32]
                    rbase[u, y0:y0 + 32, :W - dsp] = rows[:, dsp:]
                    rbase[u, y0:y0 + 32, W - dsp:] = rows[:, W - 1:W]
            rbase = np.clip(rbase.astype(np.int16) + srng.integers(-2, 3, size=rbase.shape, dtype=np.int16), 0, 255).astype(np.uint8)
            d_right = torch.from_numpy(rbase[scen["index"]]).to(dev)
            xr = pkg.Extractor(nfeatures=NF, device=local_rank)
            r_kps = torch.empty((B, cap, 7), dtype=torch.float32, device=dev)
            r_desc = torch.empty((B, cap, 32), dtype=torch.uint8, device=dev)
            r_n = torch.empty((B,), dtype=torch.int32, device=dev)
            s_ur = torch.empty((B, cap), dtype=torch.float32, device=dev)
            s_dp = torch.empty((B, cap), dtype=torch.float32, device=dev)
            mbf = np.float32(40.0)
            mb = np.float32(mbf / np.float32(517.306408))

            def stereo_step():
                # both eyes are enqueued on their own handles' streams; the stereo call waits for both
                ex.extract_batch_device_async(d_img.data_ptr(), B, W, H, W, W * H, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr())
                xr.extract_batch_device_async(d_right.data_ptr(), B, W, H, W, W * H, r_kps.data_ptr(), r_desc.data_ptr(), cap, r_n.data_ptr())
                return pkg.capi.compute_stereo_matches_device(ex, xr, B, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(),
                                                              r_kps.data_ptr(), r_desc.data_ptr(), r_n.data_ptr(), cap, mb, mbf,
                                                              s_ur.data_ptr(), s_dp.data_ptr())
            stereo_step()
            torch.cuda.synchronize()
            tb = time.perf_counter()
            sms = [stereo_step() for _ in range(5)]
            torch.cuda.synchronize()
            swall = (time.perf_counter() - tb) / 5
            extra["stereo_frontend_640x480"] = {
                "pairs_per_step": B, "pairs_per_s": B / swall, "wall_ms": swall * 1e3,
                "compute_stereo_matches_device_ms": float(np.mean(sms)), "matches_per_pair": float((s_dp > 0).sum().item()) / B}
            # rank-4 matcher rows (device time of the kernels, one call each)
            r4 = {}
            mt = pkg.Matcher(0.6, True, device=local_rank)
            tp = [S.synth_triang_problem(500 + i, 2000, 2000, n_nodes=100) for i in range(20)]
            mt.SearchForTriangulation(tp)
            mt.SearchForTriangulation(tp)
            r4["search_for_triangulation_20pairs_2000feat_ms"] = mt.last_device_ms()
            kp = [S.synth_bow_kf_problem(520 + i, 2000, 2000) for i in range(20)]
            mk = pkg.Matcher(0.75, True, device=local_rank)
            mk.SearchByBoWKF(kp)
            mk.SearchByBoWKF(kp)
            r4["search_by_bow_kf_20pairs_2000feat_ms"] = mk.last_device_ms()
            fz, pz = S.synth_proj_gen_problem(530, n_f=2000, n_pts=3000)
            mt.Fuse(fz, pz)
            mt.Fuse(fz, pz)
            r4["fuse_3000pts_2000feat_ms"] = mt.last_device_ms()
            mt.SearchByProjectionKF(fz, pz)
            mt.SearchByProjectionKF(fz, pz)
            r4["search_by_projection_kf_3000pts_ms"] = mt.last_device_ms()
            mt.SearchByProjectionReloc(fz, pz, 100)
            r4["search_by_projection_reloc_3000pts_ms"] = mt.last_device_ms()
            s1, s2, q12, q21 = S.synth_sim3_problem(540, 2000, 2000)
            mt.SearchBySim3(s1, s2, q12, q21)
            mt.SearchBySim3(s1, s2, q12, q21)
            r4["search_by_sim3_2000x2000_ms"] = mt.last_device_ms()
            oo, od = S.synth_observations(550, 4000, 24)
            mt.ComputeDistinctiveDescriptors(oo, od)
            mt.ComputeDistinctiveDescriptors(oo, od)
            r4["compute_distinctive_descriptors_4000pts_ms"] = mt.last_device_ms()
            extra["rank4_matcher"] = r4
            # ORBVocabulary::transform with a vocabulary of the real ORBvoc shape (k=10, L=6: 1.1 M nodes),
            # 64 frames x 1000 descriptors, device-resident
            voc = voc_nodes if (voc_nodes is not None and voc_nodes["L"] == 6) else S.synth_vocabulary(400, 10, 6)
            vv = pkg.Vocabulary(device=local_rank)
            vv.set_nodes(10, 6, 0, 0, voc["parent"], voc["desc"], voc["weight"], voc["is_leaf"])
            vb, vcap = 64, 1000
            vd = torch.from_numpy(np.stack([S.vocab_descriptors(rng, voc, vcap) for _ in range(4)] * (vb // 4))).to(dev)
            vn = torch.full((vb,), vcap, dtype=torch.int32, device=dev)
            v_bw = torch.empty((vb, vcap), dtype=torch.int32, device=dev)
            v_bv = torch.empty((vb, vcap), dtype=torch.float64, device=dev)
            v_fn = torch.empty((vb, vcap), dtype=torch.int32, device=dev)
            v_fo = torch.empty((vb, vcap + 1), dtype=torch.int32, device=dev)
            v_fi = torch.empty((vb, vcap), dtype=torch.int32, device=dev)
            v_nb = torch.empty((vb,), dtype=torch.int32, device=dev)
            v_nf = torch.empty((vb,), dtype=torch.int32, device=dev)
            vargs = (vb, vd.data_ptr(), vn.data_ptr(), vcap, 4, v_bw.data_ptr(), v_bv.data_ptr(), v_nb.data_ptr(),
                     v_fn.data_ptr(), v_fo.data_ptr(), v_fi.data_ptr(), v_nf.data_ptr())
            vv.transform_device(*vargs)
            vms = float(np.mean([vv.transform_device(*vargs) for _ in range(5)]))
            extra["vocabulary_transform_64frames_1000desc_k10L6"] = {
                "device_ms": vms, "descriptors_per_s": vb * vcap / (vms * 1e-3), "nodes": len(voc["parent"]) + 1,
                "words_per_frame": float(v_nb.float().mean().item())}
        except Exception as exc:  # secondary numbers must never break the contract line
            extra["error"] = repr(exc)

    if rank == 0:
        P = 1_444_097 if KITTI else 950_532  # sum of level pixels for 1241x376 / 640x480
        fast_bytes = P * B
        achieved = fast_bytes / (fast_ms * 1e-3) / 1e9
        out = headline()
        out.update({
            "stage_ms": composite_stage,
            "extractor_stage_ms": stage,
            "roofline": {"bound": "hbm", "kernel": "fast_cells_kernel", "achieved": achieved, "peak": 8000.0,
                         "unit": "GB/s", "frac": achieved / 8000.0, "traffic": None,
                         "algorithmic_bytes_per_launch": fast_bytes, "kernel_ms": fast_ms,
                         "note": "integer-VALU bound, not bandwidth bound (see roofline_valu): ~710 VALU instructions per 1.2k-pixel cell-wave at "
                                 "the issue rates measured on this chip (tools/microbench/valu_rate.hip -> profiles/r01_valu_rate.txt: 4 cycles "
                                 "per wave64 instruction for packed-16 / min / max / compare / dot / perm / mad, 2 for add / sub / logic / mov / "
                                 "f32), so the HBM fraction can only rise by removing instructions (profiles/README.md has the history: 1040 -> "
                                 "812 per cell-wave in round 1, -> 712 in round 2; round 3: the tile is staged by LDS-DMA, 0.109 -> 0.123 at "
                                 "B = 512)"},
            "extra": extra,
        })
        # the other two streaming kernels of the step, from the un-chunked stage times (HIP events of the library)
        pyr_bytes = 2.0 * P - W * H - round(W / 3.583181) * round(H / 3.583181)   # every level but the last read once, every level but the first written once (tum: 1.57e6)
        out["roofline_other"] = [
            {"kernel": "describe_kernel", "bound": "hbm", "kernel_ms": stage["describe"],
             "algorithmic_bytes_per_launch": float(n_kp.sum()) * (749 + 512 + 60),
             "achieved": float(n_kp.sum()) * (749 + 512 + 60) / (stage["describe"] * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
             "frac": float(n_kp.sum()) * (749 + 512 + 60) / (stage["describe"] * 1e-3) / 1e9 / 8000.0,
             "note": "integer-VALU bound as well (VALUBusy ~87 %, profiles/r01_pmc_sq_busy.csv): ~585 VALU instructions per keypoint "
                     "(7x7 blur of the 43x37 patch = 55 %, 512 steered samples = 20 %, IC_Angle + exact sin/cos = 20 %)"},
            {"kernel": "resize_level_kernel x7", "bound": "hbm", "kernel_ms": stage["pyramid"],
             "algorithmic_bytes_per_launch": pyr_bytes * B,
             "achieved": pyr_bytes * B / (stage["pyramid"] * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
             "frac": pyr_bytes * B / (stage["pyramid"] * 1e-3) / 1e9 / 8000.0,
             "note": "seven dependent launches (level k is resized from level k-1); the large levels run at 3.2-3.5 TB/s, the small "
                     "ones are launch / tail bound; VALUBusy 35 %"}]
        # counters of the same kernel from the committed rocprofv3 --pmc passes (B = 512 > Infinity Cache; calibrated against
        # 1 GiB copies): NOT measured in this run -- `roofline.traffic` stays null; the profiled figures are given beside it
        try:
            cnames = ("r06_extractor_counters_kitti.json",) if KITTI else ("r06_extractor_counters.json", "r05_extractor_counters.json", "r03_extractor_counters.json", "r02_extractor_counters.json")
            cpath = next((q for q in (os.path.join(ROOT, "profiles", n_) for n_ in cnames) if os.path.exists(q)), None)
            if cpath is None:
                raise LookupError("no committed PMC passes of this workload's extraction")
            pc = json.load(open(cpath))
            fc, cal = pc["fast_cells_kernel"], pc["calibration"]
            per_frame = (fc["FETCH_SIZE_KB"] * cal["FETCH_SIZE_factor_unaligned_32bit"] + fc["WRITE_SIZE_KB"] * cal["WRITE_SIZE_factor"]) * 1024.0 / pc["batch"]
            # `traffic`: HBM bytes per launch of THIS kernel on frames of THIS generator at this batch, from the committed counter passes at
            # HEAD (FETCH_SIZE / WRITE_SIZE in passes of their own, corrected as calibrated); a property of the kernel, not re-measured per run
            out["roofline"]["traffic"] = per_frame * B
            out["roofline"]["traffic_profiled"] = {
                "bytes_per_launch": per_frame * B, "over_algorithmic": per_frame * B / fast_bytes,
                "source": pc["source"], "correction": "FETCH_SIZE x %.3f (unaligned 32-bit reads), WRITE_SIZE x 1.0" % cal["FETCH_SIZE_factor_unaligned_32bit"]}
            dc = pc.get("describe_kernel")
            if dc and dc.get("FETCH_SIZE_KB"):   # describe_kernel's counter traffic beside its algorithmic bytes (1.7-1.9 x)
                d_lo = (dc["FETCH_SIZE_KB"] * cal["FETCH_SIZE_factor_unaligned_32bit"] + dc["WRITE_SIZE_KB"]) * 1024.0 / pc["batch"] * B
                d_hi = (dc["FETCH_SIZE_KB"] * cal["FETCH_SIZE_factor_aligned"] + dc["WRITE_SIZE_KB"]) * 1024.0 / pc["batch"] * B
                row = out["roofline_other"][0]
                row["traffic"] = d_hi
                row["traffic_profiled"] = {"bytes_per_launch_low_high": [d_lo, d_hi], "over_algorithmic": [d_lo / row["algorithmic_bytes_per_launch"], d_hi / row["algorithmic_bytes_per_launch"]],
                                           "source": pc["source"], "note": "FETCH_SIZE x 1.78 (all reads unaligned 4-byte) .. x 2.0 (all aligned) + WRITE_SIZE; the kernel stages a 43 x 43 patch "
                                                                           "(1849 B) per keypoint where SURVEY 8(d) counts 749 + 512 B of it: 1.40 x by construction, the rest is sector granularity "
                                                                           "(a 43-byte patch row touches two or three 32-byte sectors)"}
            insts = fc["SQ_INSTS_VALU"] / pc["batch"] * B
            clock_ghz = 2.4   # the engine clock the kernels run at (GRBM_GUI_ACTIVE / 8 / kernel time of the profiled pass gives 2.25-2.4)
            # issue cost of the kernel's instruction mix: add / sub / logic / mov / right shifts / bitop3 issue in 2 cycles per wave64
            # instruction, the packed-16 / compare / min / max / mad / perm ones in 4 (profiles/r01_valu_rate.txt); the share of each
            # class from the kernel's ISA listing (tools/isa_valu_mix.py, a static count)
            mixp = os.path.join(ROOT, "profiles", "r03_fast_isa_mix.json")
            mix = json.load(open(mixp)) if os.path.exists(mixp) else {"mean_cycles_per_instruction": 4.0, "two_cycle_share": 0.0}
            cyc = float(mix["mean_cycles_per_instruction"])
            peak = 1024 * clock_ghz / cyc   # G wave-instructions / s: 1024 SIMDs
            out["roofline_valu"] = {
                "bound": "valu_issue", "kernel": "fast_cells_kernel", "achieved": insts / (fast_ms * 1e-3) / 1e9, "peak": peak,
                "unit": "G wave64-instr/s", "frac": insts / (fast_ms * 1e-3) / 1e9 / peak,
                "mean_issue_cycles_per_instruction": cyc, "two_cycle_instruction_share": mix["two_cycle_share"],
                "frac_if_every_instruction_cost_4_cycles": insts / (fast_ms * 1e-3) / 1e9 / (1024 * clock_ghz / 4.0),
                "note": "the binding roof: instructions per launch = SQ_INSTS_VALU per frame of the committed PMC pass x B (a profiled constant of "
                        "these kernels on frames of this generator), time = this run's HIP events; peak = 1024 SIMDs x %.2f GHz / %.2f cycles per "
                        "instruction of this kernel's mix (static share of 2-cycle instructions %.0f %%; profiles/r01_valu_rate.txt).  "
                        "SQ_ACTIVE_INST_VALU ticks once per instruction whatever it costs, so a VALUBusy figure derived from it is the "
                        "4-cycle pricing, not an independent measurement" % (clock_ghz, cyc, 100.0 * mix["two_cycle_share"])}
        except Exception as exc:
            out["roofline"]["traffic_profiled"] = {"error": repr(exc)}
        try:   # the LocalBA kernels: SURVEY 8(d)'s bytes per LM iteration for the batch of this run, times and counters of the committed passes
            lpath = next((q for q in (os.path.join(ROOT, "profiles", n_) for n_ in ("r06_lba_counters.json", "r05_lba_counters.json")) if os.path.exists(q)), "")
            if not NO_LBA and not KITTI and args.lba_mix == "heterogeneous" and os.path.exists(lpath):
                lc = json.load(open(lpath))
                Np = sum(int((q_["pose_fixed"] == 0).sum()) for q_ in lba_probs); Nf = sum(int((q_["pose_fixed"] != 0).sum()) for q_ in lba_probs)
                M_ = sum(int(q_["n_points"]) for q_ in lba_probs); E_ = sum(int(q_["n_edges"]) for q_ in lba_probs)
                Ef = sum(int((q_["pose_fixed"][q_["edge_pose"]] == 0).sum()) for q_ in lba_probs)
                alg = {"k_points_walk": 56.0 * (Np + Nf) + 24.0 * M_ + 48.0 * E_ + 8.0 * (6 * Np + 3 * M_),   # residual pass + update (reads estimates / observations, writes the update)
                       "k_lin<true>": 56.0 * (Np + Nf) + 24.0 * M_ + 48.0 * E_ + 144.0 * Ef + 288.0 * Np + 72.0 * M_,   # linearisation: Hpl, Hpp, Hll
                       "k_schur": 144.0 * Ef + 72.0 * M_ + 288.0 * sum(int((q_["pose_fixed"] == 0).sum()) ** 2 for q_ in lba_probs)}   # R Hpl + Hll, W dense Hschur
                for kn, ab in alg.items():
                    kc = lc["kernels"].get(kn)
                    if kc and kc.get("kernel_us"):
                        tb = kc.get("hbm_bytes_per_launch")
                        moved = float(tb) if tb else ab   # the fraction is what the kernel MOVES (counters) over its time; SURVEY's stored-block bytes beside it
                        out["roofline_other"].append({
                            "kernel": kn, "bound": "hbm", "kernel_ms": kc["kernel_us"] * 1e-3, "algorithmic_bytes_per_launch": ab,
                            "achieved": moved / (kc["kernel_us"] * 1e-6) / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": moved / (kc["kernel_us"] * 1e-6) / 1e9 / 8000.0,
                            "frac_on_survey_stored_block_bytes": ab / (kc["kernel_us"] * 1e-6) / 1e9 / 8000.0,
                            "traffic": tb,
                            "note": "SURVEY 8(d)'s bytes per LM iteration with the stored-block layout it assumed, summed over the %d windows of this run's batch "
                                    "(the kernels keep a 32-byte record per edge instead of the 144-byte block, so the counters' traffic is below it); "
                                    "kernel time and counters: %s -- the batch alone on the device; latency / request-rate bound, not bandwidth bound" % (n_win, lc["source"][:60])})
        except Exception as exc:
            out.setdefault("roofline_notes", []).append("LocalBA rows: " + repr(exc))
        if dist_on:
            out["exchange"] = {"per_step": "gather of %d slots x %d B per rank to rank 0 (aos2_extractor_pack_slots + one collective), inside the "
                                           "timed region, in flight while the next step runs" % (B, sb),
                               "bytes_to_rank0_per_step": (world - 1) * B * sb, "backend": backend, "headers_ok": gather_ok,
                               "stream": "one of its own per pipeline, behind the step's extraction by an event",
                               "pack_plus_collective_device_us_median": float(np.median(gather["us"])) if gather["us"] else None}
        else:   # what the exchange would move at 8 ranks, and the pack kernel's own time (one launch, measured here)
            gs = torch.cuda.Stream(device=dev)
            slot_ = torch.zeros((B, sb), dtype=torch.uint8, device=dev)
            ev_ = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            with torch.cuda.stream(gs):
                pipes[0].ex.pack_slots(B, pipes[0].d_kps.data_ptr(), pipes[0].d_desc.data_ptr(), pipes[0].d_n.data_ptr(), cap, slot_.data_ptr(), sb, gs.cuda_stream)
                ev_[0].record()
                pipes[0].ex.pack_slots(B, pipes[0].d_kps.data_ptr(), pipes[0].d_desc.data_ptr(), pipes[0].d_n.data_ptr(), cap, slot_.data_ptr(), sb, gs.cuda_stream)
                ev_[1].record()
            gs.synchronize()
            out["exchange"] = {"per_step": "none at N = 1; at N ranks every rank's %d slots x %d B go to rank 0 in one gather per step (RCCL), on a stream of its "
                                           "own per pipeline behind the step's extraction" % (B, sb),
                               "slot_bytes": sb, "bytes_to_rank0_per_step_at_8_ranks": 7 * B * sb,
                               "per_xgmi_link_ms_at_8_ranks_153_GB_per_s": B * sb / 153e9 * 1e3,
                               "pack_kernel_us": ev_[0].elapsed_time(ev_[1]) * 1e3,
                               "collective_us": "measured by the one-rank RCCL path (AOS2_BENCH_FORCE_DIST=1: exchange.pack_plus_collective_device_us_median) and at N > 1"}
        co, lba_want = None, {}
        if snap is not None or (world == 1 and not args.no_cpu_baseline):
            O = g.load_oracle()
            import parity
            co = parity.ChainOracle(scen_v, pipes[jv], th_last=pipes[0].th_last, th_local=pipes[0].th_local,
                                    nnratio_local=pipes[0].nnratio_local)
        if world == 1 and not args.no_cpu_baseline:   # rank 0 at N = 1 only
            # the SAME composite through the oracle (C restatement, one core): per frame extraction + Frame members +
            # the tracking chain (oracle/chain.py), per `fpk` frames one LocalBA window (oracle lba_solve)
            n_cpu = args.cpu_frames or 32
            n_cpu = max(fpk, (n_cpu // fpk) * fpk)
            tm = {}
            co.oe.extract(scen_v["cur"][0])
            tc = time.perf_counter()
            done = 0
            for i in range(n_cpu):
                co.unique(i % n_unique, timing=tm)
                if (i + 1) % fpk == 0:
                    if voc_nodes is not None:   # the keyframe's Frame::ComputeBoW + SearchByBoW(reference keyframe, frame)
                        parity.bow_leg_mismatches(None, co, voc_nodes, [i % n_unique], timing=tm)
                    if kfws:   # LocalMapping's SearchForTriangulation + Fuse of that keyframe against its neighbours
                        co._kw_inputs = kfws[jv]
                        kb = (i // fpk) % n_bow
                        parity.keyframe_work_mismatches(None, co, voc_nodes, range(kb * kfws[jv].n_nb, (kb + 1) * kfws[jv].n_nb), timing=tm)
                    ta = time.perf_counter()
                    k = (i // fpk) % len(lba_unique)
                    lba_want[k] = O.lba_solve(lba_unique[k])
                    tm["local_ba"] = tm.get("local_ba", 0.0) + time.perf_counter() - ta
                done += 1
                if time.perf_counter() - tc - tm.get("_setup", 0.0) > 30.0 and done % fpk == 0:
                    break
            tc = time.perf_counter() - tc - tm.pop("_setup", 0.0)   # (the neighbour keyframes' own extraction is not work of the step)
            out["cpu_baseline"] = {"value": done / tc, "unit": "frames/s", "cores": 1, "kind": "port",
                                   "sample": f"{done} of the same frame pairs + {done // fpk} of the same LocalBA windows through the oracle "
                                             f"(C restatement -O3 + numpy glue, 1 thread); host has {os.cpu_count()} cores",
                                   "ms_per_frame": {k: v / done * 1e3 for k, v in tm.items()}}
            # frame-parallel all-cores number for the extractor (so that the speed-up is not inflated)
            try:
                from concurrent.futures import ThreadPoolExecutor as _TPE
                nthr = max(1, min(os.cpu_count() or 1, 64))
                exs = [O.Extractor(nfeatures=NF) for _ in range(nthr)]
                per = 4

                def work(t):
                    for i in range(per):
                        exs[t].extract(base[(t + i) % n_unique])   # (frames of pipeline 0: any frames do for this figure)
                    return per
                with _TPE(nthr) as pool2:
                    list(pool2.map(lambda t: exs[t].extract(base[t % n_unique]), range(nthr)))  # warm-up
                    ta = time.perf_counter()
                    tot = sum(pool2.map(work, range(nthr)))
                    ta = time.perf_counter() - ta
                out["cpu_baseline"]["extract_only_frame_parallel"] = {"value": tot / ta, "unit": "frames/s", "cores": nthr,
                                                                      "sample": f"{tot} frames, one oracle extractor per thread"}
            except Exception as exc:  # never break the contract line
                out["cpu_baseline"]["extract_only_frame_parallel"] = {"error": repr(exc)}
        if snap is not None:
            # ---- parity of the LAST timed step: EVERY batch position (every distinct (LastFrame, CurrentFrame) pair of the step's
            # pipeline goes through the oracle chain) and EVERY LocalBA window of the last timed batch (every distinct problem goes
            # through the oracle's solver); the oracle runs on a few host threads (its C functions hold no state)
            parity.reset_worst()
            t_or = time.perf_counter()
            n_thr = max(1, min(int(os.environ.get("AOS2_BENCH_ORACLE_THREADS", "64")), (os.cpu_count() or 1) // 2))
            t_mt = {"chain": time.perf_counter()}
            n_cached0 = len(co.cache)
            co.precompute(range(n_unique), threads=n_thr)
            t_mt["chain"] = time.perf_counter() - t_mt["chain"]
            t_mt["chain_frames"] = len(co.cache) - n_cached0
            pos = [b for b in range(B) if int(scen_v["index"][b]) in co.cache]
            bad = parity.chain_mismatches(snap["chain"], co, pos)
            if snap["lba"]:
                from concurrent.futures import ThreadPoolExecutor as _TPE2
                todo = [k for k in range(len(lba_unique)) if k not in lba_want]
                t_mt["lba"] = time.perf_counter()
                with _TPE2(n_thr) as pool3:
                    for k, w_ in zip(todo, pool3.map(lambda k_: O.lba_solve(lba_unique[k_]), todo)):
                        lba_want[k] = w_
                t_mt["lba"] = time.perf_counter() - t_mt["lba"]
                t_mt["lba_windows"] = len(todo)
            n_bow_checked = 0
            if snap["bow"] is not None:
                bpos = [b for b in range(n_bow) if int(scen_v["index"][b]) in co.cache]
                bad += parity.bow_leg_mismatches(snap["bow"], co, voc_nodes, bpos)
                n_bow_checked = len(bpos)
            n_kfw_checked = 0
            if snap["kfw"] is not None:   # every (keyframe, neighbour) pair of the step and every reverse fuse
                kq = snap["kfw"]
                kp_ = list(range(len(kq.kf1)))
                bad += parity.keyframe_work_mismatches(kq, co, voc_nodes, kp_)
                n_kfw_checked = len(kp_)
            if hb_run is not None and hb_run["snap"] is not None:   # the host-boundary run's last step (same pipeline), from its HOST arrays
                hb_run["bad"] = parity.chain_mismatches(hb_run["snap"], co, pos)
                if isinstance(out.get("extra"), dict) and out["extra"].get("composite_host_boundary"):
                    out["extra"]["composite_host_boundary"]["parity_checked_from_host_arrays"] = {
                        "ok": not hb_run["bad"], "frames": len(pos), "n_mismatches": len(hb_run["bad"]), "first": hb_run["bad"][:3]}
            if lba_hard is not None and isinstance(out.get("extra"), dict) and out["extra"].get("local_ba_batch_with_rejected_steps"):
                # every window gated: ordinary ones at 1e-5, the ones that start off the optimum at the oracle's own resolution on that
                # window (parity.lba_resolution), every decision (iterations, trials, outlier sets) the oracle's
                from concurrent.futures import ThreadPoolExecutor as _TPE3

                def _want_and_resolution(a_):
                    w__ = O.lba_solve(a_[1])
                    return w__, (parity.lba_resolution(a_[1], want=w__) if "hard" in a_[0] else None)
                with _TPE3(n_thr) as pool4:
                    hw_ = list(pool4.map(_want_and_resolution, list(zip(lba_hard["mix"], lba_hard["probs"]))))
                hbad, wp, wx, wp_h, wx_h, rp_h, rx_h = [], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
                for wi_, (m_, r_, (w_, res_)) in enumerate(zip(lba_hard["mix"], lba_hard["res"], hw_)):
                    hbad += parity.lba_mismatches(r_, w_, tag=f"LocalBA batch with rejected steps, window {wi_}", resolution=res_)
                    dp_, dx_ = float(np.abs(r_["pose_Tcw"] - w_["pose_Tcw"]).max()), float(np.abs(r_["point_xyz"] - w_["point_xyz"]).max())
                    if res_ is not None:
                        wp_h, wx_h, rp_h, rx_h = max(wp_h, dp_), max(wx_h, dx_), max(rp_h, res_["pose"]), max(rx_h, res_["point"])
                    else:
                        wp, wx = max(wp, dp_), max(wx, dx_)
                out["extra"]["local_ba_batch_with_rejected_steps"]["against_the_oracle"] = {
                    "ok": not hbad, "n_mismatches": len(hbad), "first": hbad[:3],
                    "worst_abs_diff_ordinary_windows": {"pose": wp, "point": wx},
                    "worst_abs_diff_windows_started_off_the_optimum": {"pose": wp_h, "point": wx_h},
                    "oracle_against_its_own_reassociated_runs_on_those_windows": {"pose": rp_h, "point": rx_h},
                    "rule": "iterations, trials and outlier sets of every window equal the oracle's; ordinary windows within 1e-5; a window that "
                            "starts far off: within max(1e-5, %g x the spread of the oracle against itself on that window) "
                            "(oracle/parity.py lba_resolution, profiles/r06_lba_sensitivity.txt)" % parity.LBA_RESOLUTION_FACTOR}
                bad += hbad
            wins = [w for w in range(len(snap["lba"])) if w % len(lba_unique) in lba_want]
            lba_resolutions = {}
            for w in wins:
                k_ = w % len(lba_unique)
                if lba_mix is not None and "hard" in lba_mix[k_] and k_ not in lba_resolutions:
                    lba_resolutions[k_] = parity.lba_resolution(lba_unique[k_], want=lba_want[k_])
                bad += parity.lba_mismatches(snap["lba"][w], lba_want[k_], tag=f"LocalBA window {w} (problem {k_})", resolution=lba_resolutions.get(k_))
            # BASELINE.md section 3 asks for an all-cores CPU figure beside the one-core one: the oracle's passes of this check ARE the
            # composite's per-frame chains and LocalBA windows on `n_thr` host threads (the C functions hold no state and release the
            # interpreter lock; the numpy glue between them does not, which is what limits the scaling)
            if isinstance(out.get("cpu_baseline"), dict) and t_mt.get("chain_frames", 0) > 0 and t_mt.get("lba_windows", 0) > 0:
                per_frame = t_mt["chain"] / t_mt["chain_frames"]
                per_window = t_mt["lba"] / t_mt["lba_windows"]
                one = out["cpu_baseline"].get("ms_per_frame", {})
                legs = sum(one.get(k_, 0.0) for k_ in ("compute_bow", "search_by_bow", "search_for_triangulation", "fuse")) * 1e-3   # (one thread)
                out["cpu_baseline"]["composite_frame_parallel"] = {
                    "value": 1.0 / (per_frame + per_window / fpk + legs), "unit": "frames/s", "cores": n_thr,
                    "sample": "%d distinct frame pairs through the oracle's tracking chain and %d LocalBA windows through its solver on %d threads "
                              "(the oracle passes of parity_checked), one window per %d frames; the keyframe legs at their one-thread cost" %
                              (t_mt["chain_frames"], t_mt["lba_windows"], n_thr, fpk),
                    "ms_per_frame": {"tracking_chain": per_frame * 1e3, "local_ba": per_window / fpk * 1e3, "keyframe_legs_one_thread": legs * 1e3}}
            out["parity_checked"] = {
                "ok": not bad, "step": "the last timed step (results copied right after the timed region)",
                "frames": len(pos), "distinct_frame_pairs": len(co.cache), "reference_keyframe_bow_frames": n_bow_checked,
                "keyframe_neighbour_pairs": n_kfw_checked, "local_ba_windows": len(wins),
                "distinct_local_ba_problems": len(set(w % len(lba_unique) for w in wins)),
                "worst_abs_diff": {k_: float(v_) for k_, v_ in parity.WORST.items()},
                "tolerance": "1e-5 absolute on mTcw / LocalBA poses / LocalBA points (oracle/parity.py close(): literally; a float32 of magnitude "
                             ">= 128 may differ by one float32 step instead -- no value of this workload is that large); final chi2 1e-6 relative; "
                             "a LocalBA window that STARTS off the optimum (local_ba_windows_started_off_the_optimum): max(1e-5, %g x the spread of "
                             "the oracle against its own re-associated runs on that window), every decision identical" % parity.LBA_RESOLUTION_FACTOR,
                "local_ba_windows_started_off_the_optimum": {
                    "problems": sorted(int(k_) for k_ in lba_resolutions),
                    "oracle_against_itself": {str(k_): {"pose": v_["pose"], "point": v_["point"], "decisions_equal": v_["decisions_equal"]} for k_, v_ in lba_resolutions.items()},
                    "device_against_oracle": {"pose": float(parity.WORST.get("lba_offopt_pose", 0.0)), "point": float(parity.WORST.get("lba_offopt_point", 0.0))}},
                "oracle_seconds": time.perf_counter() - t_or,
                "checked": "per frame: keypoints, descriptors, mvuRight / mvDepth, match counts of both searches, inlier counts of both "
                           "PoseOptimizations, mvpMapPoints, mvbOutlier (bit-identical), mTcw (1e-5); per keyframe frame: the SearchByBoW match "
                           "array and count behind ComputeBoW (bit-identical); per (keyframe, neighbour) pair: vMatches12 and count of "
                           "SearchForTriangulation, best index / distance of Fuse's search, both directions (bit-identical); per window: iteration and trial "
                           "counts, outlier sets (identical), poses and points (1e-5), final chi2 (1e-6 relative)",
                "against": "oracle (C restatement; parity unpinned by the reference: DESIGN.md section 3)",
                "mismatches": bad[:10], "n_mismatches": len(bad)}
        print(json.dumps(out))
        if snap is not None and not out["parity_checked"]["ok"]:
            sys.stdout.flush()
            raise SystemExit(3)   # a fast wrong result is not a result
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
