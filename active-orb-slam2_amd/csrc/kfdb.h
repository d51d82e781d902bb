// The arithmetic and the decisions of KeyFrameDatabase (src/KeyFrameDatabase.cc:76-309) that the device kernels (csrc/kfdb.hip)
// and the host tap (aos2_debug_kfdb_host) share: the L1 score term and its cast (L1Scoring::score, ScoringObject.cpp:23-72, through
// TemplatedVocabulary::score :1191-1195), the common-word cut (:120 / :235), the order key of lKFsSharingWords, the accumulation
// over the covisibility neighbours (:148-173 / :262-287) and the retain threshold (:176 / :290).  ONE routine set: the translation
// unit is built with -ffp-contract=off, there is no libm call but fabs, so both sides run the same operation sequence and every
// output is derivable bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/aos2.h"

namespace aos2 {

// one common word of L1Scoring::score: vi = the query's value (the FIRST argument of score), wi = the slot's
__host__ __device__ inline double kfdb_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }

// `s` = the terms of the common words added in ascending word id, starting from 0.0 -> float si (:133 / :249)
__host__ __device__ inline float kfdb_score(double s) { return (float)(-s / 2.0); }

// int minCommonWords = maxCommonWords*0.8f (:120 / :235): a float product, truncated
__host__ __device__ inline int kfdb_min_common(int max_common_words) { return (int)(max_common_words * 0.8f); }

// float minScoreToRetain = 0.75f*bestAccScore (:176 / :290)
__host__ __device__ inline float kfdb_retain(float best_acc_score) { return 0.75f * best_acc_score; }

// lKFsSharingWords is in order of first encounter: ascending (first common word, position in that word's inverted list), and
// the position is add order.  `rank` = the slot's place among the added slots in add order.
__host__ __device__ inline uint64_t kfdb_key(uint32_t first_common_word, uint32_t rank)
{
    return ((uint64_t)first_common_word << 32) | rank;
}

// position of `w` in the ascending row, -1 if absent
__host__ __device__ inline int kfdb_find(const uint32_t *row, int n, uint32_t w)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && row[lo] == w) ? lo : -1;
}

// the sum of L1Scoring::score over two ascending BowVectors, v1 = the query: the host form of the walk (a merge)
__host__ __device__ inline double kfdb_merge_sum(const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2,
                                                int n2)
{
    int i = 0, j = 0;
    double s = 0;
    while (i < n1 && j < n2) {
        if (w1[i] == w2[j]) {
            s += kfdb_term(v1[i], v2[j]);
            ++i;
            ++j;
        } else if (w1[i] < w2[j]) {
            ++i;
        } else {
            ++j;
        }
    }
    return s;
}

// One entry of lScoreAndMatch (:148-173 / :262-287): the slot `self` with its score si and its neighbour row
// (GetBestCovisibilityKeyFrames(10), -1 padded).  look(slot, value) says whether the neighbour takes part and with which score
// (LOOP: scored in this query; RELOC: shares a word, and then mRelocScore as it stands).
template <class Look>
__host__ __device__ inline void kfdb_accumulate(float si, int32_t self, const int32_t *neigh, const Look &look, float &acc_score,
                                                int32_t &best_slot)
{
    float best_score = si;
    acc_score = si;
    best_slot = self;
    for (int k = 0; k < AOS2_KFDB_NEIGHBOURS; ++k) {
        float s2;
        if (neigh[k] < 0 || !look(neigh[k], s2)) continue;
        acc_score += s2;
        if (s2 > best_score) {
            best_slot = neigh[k];
            best_score = s2;
        }
    }
}

}  // namespace aos2
