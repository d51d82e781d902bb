"""Stage driver: device time of aos2_frames_triangulate_matches at the bench's keyframe shape (64 keyframes x 10 neighbours,
TUM-shaped frames, matches from chain.KeyFrameWork), from HIP events around the call on the handle's stream; one JSON line.
Per kernel: rocprofv3 --kernel-trace --stats -- python tools/gpu_triangulate_prof.py (a run of its own).  TRI_REPS = timed calls,
AOS2_LIB = another build of the library to compare with."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
pkg = g.load_package()
scen = pkg.scenario.tracking_scenario(100, 64, cfg="tum", n_unique=64)
tc = pkg.chain.TrackingChain(scen, n_local=1500)
voc = pkg.synth.synth_vocabulary(400, 10, 6)
kw = pkg.chain.KeyFrameWork(tc, voc, n_kf=64, n_nb=10).run()
kw.triangulate()
ext = torch.cuda.ExternalStream(tc.last.stream(), device=tc.dev)
times = []
n_rep = int(os.environ.get("TRI_REPS", "30"))
for it in range(n_rep + 5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ext)
    tc.last.TriangulateMatches(kw.kfs, kw.t_kf1, kw.t_kf2, kw.d_match12.data_ptr(), kw.d_x3D.data_ptr(), kw.d_tri_status.data_ptr(),
                               kw.d_nnew.data_ptr(), first_wins=True)
    e1.record(ext)
    tc.last.wait()
    torch.cuda.synchronize()
    if it >= 5:
        times.append(e0.elapsed_time(e1))
st = kw.tri_status
out = dict(lib=os.environ.get("AOS2_LIB", "default"), pairs=int(len(kw.t_kf1)), cap=int(tc.cap), matched=int((kw.match12 >= 0).sum()),
           matched_per_pair=float((kw.match12 >= 0).sum(1).mean()), accepted=int((st == 1).sum()), superseded=int((st == 10).sum()),
           status_hist=np.bincount(st.ravel(), minlength=11).tolist(), nnew_total=int(kw.nnew.sum()),
           event_ms_median=float(np.median(times)), event_ms_min=float(np.min(times)), event_ms_max=float(np.max(times)),
           x3D_crc=int(np.frombuffer(kw.x3D.tobytes(), np.uint32).sum() & 0xffffffff))
print(json.dumps(out))
