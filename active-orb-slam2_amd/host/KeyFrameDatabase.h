// ORB_SLAM2::KeyFrameDatabase at the reference's signatures (include/KeyFrameDatabase.h:42-70, src/KeyFrameDatabase.cc), for the
// call sites that stay as they are: Tracking::Relocalization (src/Tracking.cc:1528), LoopClosing::DetectLoop
// (src/LoopClosing.cc:143), LocalMapping / KeyFrame::SetBadFlag (add / erase) and Tracking::Reset (clear).
//
// The inverted file is gone: a KeyFrame* maps to a SLOT of an aos2_kfdb_t (its BowVector resident on the device, put when the
// class first sees the keyframe), and a query is ONE C-ABI call (aos2_kfdb_detect) that returns the sharing list (the keyframes
// of lKFsSharingWords with their word counts) and the scored list (those above the common-word cut with their scores), both in
// the reference's list order.  From them the class writes the members the reference's walk leaves behind -- mnLoopQuery,
// mnLoopWords, mLoopScore or mnRelocQuery, mnRelocWords, mRelocScore of the sharing keyframes that are not connected to the query
// -- and then accumulates over the covisibility neighbours on the pointer graph, with the live GetBestCovisibilityKeyFrames(10)
// and the members as they stand (:144-196 / :258-308): no neighbour table has to be kept fresh on the device, and a neighbour's
// stale mRelocScore is the keyframe's own member, as in the reference.
//
// What differs from the reference, by construction: the connected keyframes of a loop query keep their mnLoopWords (the
// reference's walk counts into them without ever reading the count), and mMutex is held for the whole query instead of for the
// walk (the call IS the walk).
// Include AFTER the headers that declare KeyFrame, Frame, DBoW2::BowVector (the reference's, or tests/cpp/refstub/kfdb_stub.h)
// and after ORBVocabulary.h of this directory.
#pragma once
#include <cstdint>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "aos2_handles.h"

namespace ORB_SLAM2 {

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary &voc) : mpVoc(&voc)
    {
        aos2::check(aos2_kfdb_create(voc.handle(), aos2::thread_device(), &mpDb), "KeyFrameDatabase");
    }
    ~KeyFrameDatabase() { aos2_kfdb_destroy(mpDb); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    void add(KeyFrame *pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        aos2::check(aos2_kfdb_add(mpDb, SlotOf(pKF)), "KeyFrameDatabase::add");
    }

    void erase(KeyFrame *pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        std::map<KeyFrame *, int32_t>::iterator it = mSlotOf.find(pKF);
        if (it != mSlotOf.end()) aos2::check(aos2_kfdb_erase(mpDb, it->second), "KeyFrameDatabase::erase");
    }

    void clear() { aos2::check(aos2_kfdb_clear(mpDb), "KeyFrameDatabase::clear"); }

    // Loop Detection
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore)
    {
        std::set<KeyFrame *> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
        Lists L;
        {
            std::unique_lock<std::mutex> lock(mMutex);
            std::vector<int32_t> excluded;
            for (std::set<KeyFrame *>::iterator sit = spConnectedKeyFrames.begin(); sit != spConnectedKeyFrames.end(); ++sit) {
                std::map<KeyFrame *, int32_t>::iterator it = mSlotOf.find(*sit);
                if (it != mSlotOf.end()) excluded.push_back(it->second);
            }
            aos2_kfdb_query_t Q = {};
            Q.mode = AOS2_KFDB_LOOP;
            Q.slot = SlotOf(pKF);
            Q.min_score = minScore;
            Q.n_excluded = (int32_t)excluded.size();
            Q.excluded = excluded.data();
            Detect(Q, L);
            for (size_t i = 0; i < L.sharing.size(); ++i) {   // what :86-104 leaves in the keyframes it lists
                KeyFrame *pKFi = mvpKeyFrames[L.sharing[i]];
                pKFi->mnLoopQuery = pKF->mnId;
                pKFi->mnLoopWords = L.sharing_words[i];
            }
        }
        std::list<std::pair<float, KeyFrame *> > lScoreAndMatch;
        for (size_t i = 0; i < L.scored.size(); ++i) {        // :125-139
            KeyFrame *pKFi = mvpKeyFrames[L.scored[i]];
            pKFi->mLoopScore = L.score[i];
            if (L.score[i] >= minScore) lScoreAndMatch.push_back(std::make_pair(L.score[i], pKFi));
        }
        const int minCommonWords = L.min_common_words;
        const long unsigned int id = pKF->mnId;
        return Accumulate(lScoreAndMatch, minScore, [minCommonWords, id](KeyFrame *pKF2, float &score) {
            if (pKF2->mnLoopQuery != id || pKF2->mnLoopWords <= minCommonWords) return false;
            score = pKF2->mLoopScore;
            return true;
        });
    }

    // Relocalization
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F)
    {
        Lists L;
        {
            std::unique_lock<std::mutex> lock(mMutex);
            std::vector<uint32_t> words;
            std::vector<double> values;
            Rows(F->mBowVec, words, values);
            aos2_kfdb_query_t Q = {};
            Q.mode = AOS2_KFDB_RELOC;
            Q.slot = -1;
            Q.words = words.data();
            Q.values = values.data();
            Q.n_words = (int32_t)words.size();
            Detect(Q, L);
            for (size_t i = 0; i < L.sharing.size(); ++i) {   // :207-222
                KeyFrame *pKFi = mvpKeyFrames[L.sharing[i]];
                pKFi->mnRelocQuery = F->mnId;
                pKFi->mnRelocWords = L.sharing_words[i];
            }
        }
        std::list<std::pair<float, KeyFrame *> > lScoreAndMatch;
        for (size_t i = 0; i < L.scored.size(); ++i) {        // :242-253
            KeyFrame *pKFi = mvpKeyFrames[L.scored[i]];
            pKFi->mRelocScore = L.score[i];
            lScoreAndMatch.push_back(std::make_pair(L.score[i], pKFi));
        }
        const long unsigned int id = F->mnId;
        return Accumulate(lScoreAndMatch, 0.0f, [id](KeyFrame *pKF2, float &score) {
            if (pKF2->mnRelocQuery != id) return false;
            score = pKF2->mRelocScore;   // as it stands: stale if this query did not score pKF2
            return true;
        });
    }

protected:
    struct Lists {
        std::vector<int32_t> sharing, sharing_words, scored, scored_words;
        std::vector<float> score;
        int min_common_words = 0;
    };

    static void Rows(const DBoW2::BowVector &v, std::vector<uint32_t> &words, std::vector<double> &values)
    {
        words.reserve(v.size());
        values.reserve(v.size());
        for (DBoW2::BowVector::const_iterator vit = v.begin(); vit != v.end(); ++vit) {
            words.push_back(vit->first);
            values.push_back(vit->second);
        }
    }

    // the keyframe's slot; its BowVector goes to the device the first time the class sees it (mMutex held)
    int32_t SlotOf(KeyFrame *pKF)
    {
        std::map<KeyFrame *, int32_t>::iterator it = mSlotOf.find(pKF);
        if (it != mSlotOf.end()) return it->second;
        std::vector<uint32_t> words;
        std::vector<double> values;
        Rows(pKF->mBowVec, words, values);
        int32_t slot = -1;
        aos2::check(aos2_kfdb_put(mpDb, words.data(), values.data(), (int)words.size(), &slot), "KeyFrameDatabase");
        mSlotOf[pKF] = slot;
        if ((size_t)slot >= mvpKeyFrames.size()) mvpKeyFrames.resize((size_t)slot + 1, nullptr);
        mvpKeyFrames[slot] = pKF;
        return slot;
    }

    // ONE call: the sharing list and the scored list of the query (mMutex held)
    void Detect(const aos2_kfdb_query_t &Q, Lists &L)
    {
        const int n = aos2_kfdb_size(mpDb);
        L.sharing.resize(n); L.sharing_words.resize(n); L.scored.resize(n); L.scored_words.resize(n); L.score.resize(n);
        std::vector<int32_t> candidates(n);
        aos2_kfdb_result_t R = {};
        R.candidates = candidates.data();
        R.scored_slot = L.scored.data();
        R.scored_words = L.scored_words.data();
        R.scored_score = L.score.data();
        R.sharing_slot = L.sharing.data();
        R.sharing_words = L.sharing_words.data();
        R.cap_candidates = R.cap_scored = R.cap_sharing = n;
        aos2::check(aos2_kfdb_detect(mpDb, &Q, &R, 1), "KeyFrameDatabase");
        L.sharing.resize(R.n_sharing); L.sharing_words.resize(R.n_sharing);
        L.scored.resize(R.n_scored); L.scored_words.resize(R.n_scored); L.score.resize(R.n_scored);
        L.min_common_words = R.min_common_words;
    }

    // :141-196 / :255-308 on the pointer graph.  takes(pKF2, score): whether the neighbour takes part, and with which score.
    template <class Takes>
    static std::vector<KeyFrame *> Accumulate(const std::list<std::pair<float, KeyFrame *> > &lScoreAndMatch, float bestAccScore,
                                              const Takes &takes)
    {
        if (lScoreAndMatch.empty()) return std::vector<KeyFrame *>();
        std::list<std::pair<float, KeyFrame *> > lAccScoreAndMatch;
        for (std::list<std::pair<float, KeyFrame *> >::const_iterator it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); ++it) {
            KeyFrame *pBestKF = it->second;
            float bestScore = it->first, accScore = it->first;
            const std::vector<KeyFrame *> vpNeighs = it->second->GetBestCovisibilityKeyFrames(10);
            for (size_t k = 0; k < vpNeighs.size(); ++k) {
                float score2;
                if (!takes(vpNeighs[k], score2)) continue;
                accScore += score2;
                if (score2 > bestScore) {
                    pBestKF = vpNeighs[k];
                    bestScore = score2;
                }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        const float minScoreToRetain = 0.75f * bestAccScore;
        std::set<KeyFrame *> spAlreadyAddedKF;
        std::vector<KeyFrame *> vpCandidates;
        vpCandidates.reserve(lAccScoreAndMatch.size());
        for (std::list<std::pair<float, KeyFrame *> >::iterator it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end(); ++it)
            if (it->first > minScoreToRetain && spAlreadyAddedKF.insert(it->second).second) vpCandidates.push_back(it->second);
        return vpCandidates;
    }

    // Associated vocabulary
    const ORBVocabulary *mpVoc;

    // the device-resident database, and KeyFrame* <-> slot
    aos2_kfdb_t *mpDb = nullptr;
    std::map<KeyFrame *, int32_t> mSlotOf;
    std::vector<KeyFrame *> mvpKeyFrames;

    // Mutex
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2
