"""KeyFrame::UpdateConnections (src/KeyFrame.cc:350-440) restated in plain Python with dicts, from the reference's text alone: the
counting stage and the ordering, per keyframe.  A graph is a dict with the fields of aos2_local_map_graph_t.  Keyframe pointers are
rows: ascending row stands for pointer order (the iteration order of map<KeyFrame*, int>, the tie-break of sort on pair<int,
KeyFrame*>).  Shares no code with csrc/connections.h."""
import numpy as np

TH = 15


def update_connections_one(g, kf, matches, th=TH):
    """one keyframe: kf = its row (-1: not in the graph, nothing is skipped); matches = GetMapPointMatches() as rows (-1 = NULL) ->
    (KFcounter as {row: weight}, [(row, weight)] = mvpOrderedConnectedKeyFrames with mvOrderedWeights)"""
    obs_off, obs_kf, bad, n_points = g["obs_off"], g["obs_kf"], g["point_bad"], g["n_points"]
    KFcounter = {}
    for pMP in matches:                       # :363
        pMP = int(pMP)
        if pMP < 0:                           # :367  if(!pMP) continue
            continue
        if pMP >= n_points:                   # a point the table does not know
            continue
        if bad[pMP]:                          # :370  if(pMP->isBad()) continue
            continue
        for e in range(int(obs_off[pMP]), int(obs_off[pMP + 1])):   # :373-380
            other = int(obs_kf[e])
            if other == kf:                   # :375  mit->first->mnId == mnId
                continue
            KFcounter[other] = KFcounter.get(other, 0) + 1
    if not KFcounter:                         # :384
        return {}, []
    nmax, pKFmax = 0, None
    vPairs = []
    for row in sorted(KFcounter):             # :395  the map's iteration order
        w = KFcounter[row]
        if w > nmax:                          # :397  strictly more: the first maximum stays
            nmax, pKFmax = w, row
        if w >= th:                           # :402
            vPairs.append((w, row))
    if not vPairs:                            # :409
        vPairs.append((nmax, pKFmax))
    vPairs.sort()                             # :415  on (weight, pointer), ascending
    ordered = []
    for w, row in vPairs:                     # :418-422  push_front
        ordered.insert(0, (row, w))
    return KFcounter, ordered


def resident_matches(g, kf):
    return [int(v) for v in g["kf_mp"][g["kf_mp_off"][kf]:g["kf_mp_off"][kf + 1]]]


def update_connections(g, kf, mp=None, th=TH, conn_cap=256, ordered_cap=256):
    """the batch in the shape of the C call: kf = rows, mp = None (the resident matches) or a list of match lists ->
    dict(n_conn, n_ordered [n], conn_kf, conn_w [n][conn_cap], ordered_kf, ordered_w [n][ordered_cap], counters, ordered: the
    untruncated results per keyframe)"""
    n = len(kf)
    out = dict(n_conn=np.zeros(n, np.int32), n_ordered=np.zeros(n, np.int32),
               conn_kf=np.full((n, conn_cap), -1, np.int32), conn_w=np.zeros((n, conn_cap), np.int32),
               ordered_kf=np.full((n, ordered_cap), -1, np.int32), ordered_w=np.zeros((n, ordered_cap), np.int32), counters=[], ordered=[])
    for k in range(n):
        row = int(kf[k])
        counter, ordered = update_connections_one(g, row, resident_matches(g, row) if mp is None else mp[k], th)
        out["counters"].append(counter)
        out["ordered"].append(ordered)
        out["n_conn"][k], out["n_ordered"][k] = len(counter), len(ordered)
        for j, r in enumerate(sorted(counter)[:conn_cap]):
            out["conn_kf"][k, j], out["conn_w"][k, j] = r, counter[r]
        for j, (r, w) in enumerate(ordered[:ordered_cap]):
            out["ordered_kf"][k, j], out["ordered_w"][k, j] = r, w
    return out
