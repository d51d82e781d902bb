// The body of ORB_SLAM2::Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:782-1045) at the signature Optimizer.h declares:
// :798-984 stay as a gather -- vScw, the four kinds of edges in the reference's order with Sji = Sjw * Swi formed by g2o::Sim3's own
// arithmetic, the map points' reference keyframes (:1021-1030) -- ONE C-ABI call (aos2_optimize_essential_graph) replaces the g2o
// graph and optimize(20) with the recovery arithmetic of :1000-1008 and :1033-1040, and the results go back under
// pMap->mMutexMapUpdate in the reference's order.  LoopClosing::CorrectLoop (src/LoopClosing.cc:569) calls it unchanged.
// Keyframes with isBad() are skipped in all three loops (the reference skips them in the first only and would dereference a null
// vertex in the third; Map::GetAllKeyFrames never returns one: DESIGN.md section 2 item 14).
// Include AFTER LoopClosing.h, Converter.h, g2o's types/sim3.h and Optimizer.h.
#pragma once
#include "Optimizer.h"

namespace ORB_SLAM2 {

inline void Optimizer::OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                              const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                              const std::map<KeyFrame *, std::set<KeyFrame *>> &LoopConnections, const bool &bFixScale)
{
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();
    const unsigned int nMaxKFid = pMap->GetMaxKFid();

    std::vector<g2o::Sim3> vScw(nMaxKFid + 1);
    std::vector<int32_t> vertex_of(nMaxKFid + 1, -1);   // mnId -> vertex index: the not-bad keyframes in ascending mnId (g2o's hessian order)
    const int minFeat = 100;

    // Set KeyFrame vertices (:810-845)
    std::vector<KeyFrame *> vpVertexKF;
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int nIDi = pKF->mnId;
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end())
            vScw[nIDi] = it->second;
        else
            vScw[nIDi] = g2o::Sim3(Converter::toMatrix3d(pKF->GetRotation()), Converter::toVector3d(pKF->GetTranslation()), 1.0);
        vpVertexKF.push_back(pKF);
    }
    std::sort(vpVertexKF.begin(), vpVertexKF.end(), [](KeyFrame *a, KeyFrame *b) { return a->mnId < b->mnId; });
    for (size_t i = 0; i < vpVertexKF.size(); ++i) vertex_of[vpVertexKF[i]->mnId] = (int32_t)i;

    std::vector<int32_t> v0, v1;
    std::vector<double> Sji8, Scw8;
    auto put = [](std::vector<double> &dst, const g2o::Sim3 &S) {
        dst.push_back(S.rotation().x()); dst.push_back(S.rotation().y()); dst.push_back(S.rotation().z()); dst.push_back(S.rotation().w());
        for (int k = 0; k < 3; ++k) dst.push_back(S.translation()[k]);
        dst.push_back(S.scale());
    };
    auto add_edge = [&](long unsigned int nIDi, long unsigned int nIDj, const g2o::Sim3 &Sji) {   // vertex 0 = nIDi, vertex 1 = nIDj
        v0.push_back(vertex_of[nIDi]);
        v1.push_back(vertex_of[nIDj]);
        put(Sji8, Sji);
    };
    for (size_t i = 0; i < vpVertexKF.size(); ++i) put(Scw8, vScw[vpVertexKF[i]->mnId]);

    std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;

    // Set Loop edges (:853-881)
    for (std::map<KeyFrame *, std::set<KeyFrame *>>::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        if (pKF->isBad()) continue;
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame *> &spConnections = mit->second;
        const g2o::Sim3 Siw = vScw[nIDi];
        const g2o::Sim3 Swi = Siw.inverse();
        for (std::set<KeyFrame *>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            if ((*sit)->isBad()) continue;
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            const g2o::Sim3 Sjw = vScw[nIDj];
            const g2o::Sim3 Sji = Sjw * Swi;
            add_edge(nIDi, nIDj, Sji);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }

    // Set normal edges (:884-984)
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int nIDi = pKF->mnId;
        g2o::Sim3 Swi;
        LoopClosing::KeyFrameAndPose::const_iterator iti = NonCorrectedSim3.find(pKF);
        if (iti != NonCorrectedSim3.end())
            Swi = (iti->second).inverse();
        else
            Swi = vScw[nIDi].inverse();
        auto Sxw = [&](KeyFrame *pKFx) {   // NonCorrectedSim3 where the keyframe has one, vScw otherwise (:908-913, :935-940, :966-971)
            LoopClosing::KeyFrameAndPose::const_iterator itx = NonCorrectedSim3.find(pKFx);
            return itx != NonCorrectedSim3.end() ? itx->second : vScw[pKFx->mnId];
        };

        KeyFrame *pParentKF = pKF->GetParent();
        // Spanning tree edge
        if (pParentKF && !pParentKF->isBad()) add_edge(nIDi, pParentKF->mnId, Sxw(pParentKF) * Swi);

        // Loop edges
        const std::set<KeyFrame *> sLoopEdges = pKF->GetLoopEdges();
        for (std::set<KeyFrame *>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrame *pLKF = *sit;
            if (pLKF->mnId < pKF->mnId && !pLKF->isBad()) add_edge(nIDi, pLKF->mnId, Sxw(pLKF) * Swi);
        }

        // Covisibility graph edges
        const std::vector<KeyFrame *> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (std::vector<KeyFrame *>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame *pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    add_edge(nIDi, pKFn->mnId, Sxw(pKFn) * Swi);
                }
            }
        }
    }

    // the map points that are not bad and their reference keyframes (:1014-1030)
    std::vector<MapPoint *> vpPoints;
    std::vector<float> Xw;
    std::vector<int32_t> ref;
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId)
            nIDr = pMP->mnCorrectedReference;
        else
            nIDr = pMP->GetReferenceKeyFrame()->mnId;
        const cv::Mat P3Dw = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) Xw.push_back(P3Dw.at<float>(k));
        ref.push_back(vertex_of[nIDr]);
        vpPoints.push_back(pMP);
    }

    const size_t nv = vpVertexKF.size(), np = vpPoints.size();
    std::vector<double> Scw_out(8 * nv + 8);
    std::vector<float> Tiw_out(16 * nv + 16), Xw_out(3 * np + 3);
    aos2_essential_graph_problem_t P;
    memset(&P, 0, sizeof(P));
    P.n_vertices = (int32_t)nv;
    P.Scw = Scw8.data();
    P.fixed = vertex_of[pLoopKF->mnId];
    P.n_edges = (int32_t)v0.size();
    P.v0 = v0.data(); P.v1 = v1.data(); P.Sji = Sji8.data();
    P.fix_scale = bFixScale ? 1 : 0;
    P.iterations = 20;
    P.n_points = (int32_t)np;
    P.Xw = Xw.data(); P.ref = ref.data();
    aos2_essential_graph_result_t R;
    memset(&R, 0, sizeof(R));
    R.Scw = Scw_out.data(); R.Tiw = Tiw_out.data(); R.Xw = Xw_out.data();
    if (aos2_optimize_essential_graph(aos2::optimizer_handle(), &P, &R, 1) != AOS2_OK) {
        aos2::report("OptimizeEssentialGraph");   // the map stays as it was: the loop is closed by the fused points and the new edges alone
        return;
    }

    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);

    // SE3 Pose Recovering (:993-1011)
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKFi = vpKFs[i];
        if (pKFi->isBad()) continue;
        const float *T = Tiw_out.data() + 16 * (size_t)vertex_of[pKFi->mnId];
        cv::Mat Tiw(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tiw.at<float>(r, c) = T[4 * r + c];
        pKFi->SetPose(Tiw);
    }

    // Correct points (:1014-1044)
    for (size_t k = 0; k < np; ++k) {
        cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) cvCorrectedP3Dw.at<float>(r) = Xw_out[3 * k + r];
        vpPoints[k]->SetWorldPos(cvCorrectedP3Dw);
        vpPoints[k]->UpdateNormalAndDepth();
    }
}

}  // namespace ORB_SLAM2
