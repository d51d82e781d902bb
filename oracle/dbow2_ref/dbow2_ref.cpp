// TEST INFRASTRUCTURE: driver around the reference's own DBoW2 sources (compiled untouched by the `dbow2_ref`
// target of oracle/Makefile; nothing of them is in this repository).  One invocation loads a vocabulary file and
// records what the reference computes from it:
//
//   dbow2_ref <in.bundle> <out.bundle>          (bundle layout: tests/cpp/bundle_io.h, tests/bundle_io.py)
//
// in:  voc_path u8[], binary i32            the file and which loader reads it (0 loadFromTextFile, 1 loadFromBinaryFile)
//      pre_path u8[], pre_binary i32        optional: a file loaded first (the state a refused load is left in)
//      set_scoring i32, set_weighting i32   optional, -1 = keep the file's: setScoringType / setWeightingType
//      desc u8[N][32], set_off i32[S+1], levelsup i32[S]   S descriptor sets
//      pairs i32[P][2]                      set indices to score()
//      save i32                             optional, != 0: also return the bytes of saveToBinaryFile
// out: loaded, size, n_nodes, k, L, scoring, weighting (i32), node_parent / node_leaf / node_word i32[n_nodes],
//      node_weight f64[n_nodes], node_desc u8[n_nodes][32] (zeros where the node has no descriptor),
//      per set s: "s<s>.bow_word" i32, "s<s>.bow_value" f64, "s<s>.fv_node" i32, "s<s>.fv_off" i32, "s<s>.fv_idx" i32
//      (transform(features, BowVector, FeatureVector, levelsup)), "s<s>.word_of" / "s<s>.node_of" i32 and
//      "s<s>.weight_of" f64 (the five-argument transform per feature; node_of starts as -1, which is what stays
//      where the reference never assigns *nid), score f64[P], saved u8[].
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"
#include "bundle_io.h"

namespace {

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> RefVocabulary;

struct Voc : RefVocabulary {
    void report(Bundle &out) const
    {
        const size_t nn = m_nodes.size();
        std::vector<int32_t> parent(nn), leaf(nn), word(nn);
        std::vector<double> weight(nn);
        std::vector<uint8_t> desc(nn * 32, 0);
        for (size_t i = 0; i < nn; ++i) {
            parent[i] = (int32_t)m_nodes[i].parent;
            leaf[i] = m_nodes[i].isLeaf() ? 1 : 0;
            word[i] = (int32_t)m_nodes[i].word_id;
            weight[i] = m_nodes[i].weight;
            if (!m_nodes[i].descriptor.empty()) memcpy(&desc[i * 32], m_nodes[i].descriptor.data, 32);
        }
        out.put("node_parent", 1, parent);
        out.put("node_leaf", 1, leaf);
        out.put("node_word", 1, word);
        out.put("node_weight", 4, weight);
        out.put("node_desc", 0, desc, {(uint64_t)nn, 32});
        out.put("size", 1, std::vector<int32_t>{(int32_t)size()});
        out.put("n_nodes", 1, std::vector<int32_t>{(int32_t)nn});
        out.put("k", 1, std::vector<int32_t>{m_k});
        out.put("L", 1, std::vector<int32_t>{m_L});
        out.put("scoring", 1, std::vector<int32_t>{(int32_t)m_scoring});
        out.put("weighting", 1, std::vector<int32_t>{(int32_t)m_weighting});
    }
    void one(const cv::Mat &f, DBoW2::WordId &w, DBoW2::WordValue &v, DBoW2::NodeId *nid, int levelsup) const
    {
        RefVocabulary::transform(f, w, v, nid, levelsup);
    }
};

std::string text_of(const BundleArray &a) { return std::string(a.as<char>(), a.count()); }

bool load(Voc &voc, const std::string &path, int binary)
{
    return binary ? voc.loadFromBinaryFile(path) : voc.loadFromTextFile(path);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: dbow2_ref <in.bundle> <out.bundle>\n");
        return 2;
    }
    try {
        const Bundle in = Bundle::load(argv[1]);
        Bundle out;
        Voc voc;
        if (in.has("pre_path")) load(voc, text_of(in["pre_path"]), in["pre_binary"].scalar<int32_t>());
        const bool ok = load(voc, text_of(in["voc_path"]), in["binary"].scalar<int32_t>());
        out.put("loaded", 1, std::vector<int32_t>{ok ? 1 : 0});
        if (in.has("set_scoring") && in["set_scoring"].scalar<int32_t>() >= 0)
            voc.setScoringType((DBoW2::ScoringType)in["set_scoring"].scalar<int32_t>());
        if (in.has("set_weighting") && in["set_weighting"].scalar<int32_t>() >= 0)
            voc.setWeightingType((DBoW2::WeightingType)in["set_weighting"].scalar<int32_t>());
        voc.report(out);

        const int S = in.has("levelsup") ? (int)in["levelsup"].count() : 0;
        std::vector<DBoW2::BowVector> bows((size_t)S);
        for (int s = 0; s < S; ++s) {
            const int32_t *off = in["set_off"].as<int32_t>();
            const int levelsup = in["levelsup"].as<int32_t>()[s];
            const int n = off[s + 1] - off[s];
            std::vector<cv::Mat> feats((size_t)n);
            for (int i = 0; i < n; ++i) {
                feats[i].create(1, 32, CV_8U);
                memcpy(feats[i].data, in["desc"].as<uint8_t>() + (size_t)(off[s] + i) * 32, 32);
            }
            DBoW2::FeatureVector fv;
            voc.transform(feats, bows[s], fv, levelsup);
            std::vector<int32_t> bw, fn, fo, fi, wo((size_t)n, 0), no((size_t)n, -1);
            std::vector<double> bv, wt((size_t)n, 0.0);
            for (DBoW2::BowVector::const_iterator it = bows[s].begin(); it != bows[s].end(); ++it) {
                bw.push_back((int32_t)it->first);
                bv.push_back(it->second);
            }
            fo.push_back(0);
            for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
                fn.push_back((int32_t)it->first);
                for (unsigned int f : it->second) fi.push_back((int32_t)f);
                fo.push_back((int32_t)fi.size());
            }
            if (!voc.empty())
                for (int i = 0; i < n; ++i) {
                    DBoW2::WordId w = 0;
                    DBoW2::WordValue v = 0;
                    DBoW2::NodeId nid = (DBoW2::NodeId)-1;
                    voc.one(feats[i], w, v, &nid, levelsup);
                    wo[i] = (int32_t)w;
                    no[i] = (int32_t)nid;
                    wt[i] = v;
                }
            const std::string p = "s" + std::to_string(s) + ".";
            out.put(p + "bow_word", 1, bw);
            out.put(p + "bow_value", 4, bv);
            out.put(p + "fv_node", 1, fn);
            out.put(p + "fv_off", 1, fo);
            out.put(p + "fv_idx", 1, fi);
            out.put(p + "word_of", 1, wo);
            out.put(p + "node_of", 1, no);
            out.put(p + "weight_of", 4, wt);
        }
        if (in.has("pairs")) {
            const int P = (int)in["pairs"].dims[0];
            std::vector<double> sc((size_t)P);
            for (int p = 0; p < P; ++p) {
                const int32_t *ab = in["pairs"].as<int32_t>() + 2 * p;
                sc[p] = voc.score(bows[ab[0]], bows[ab[1]]);
            }
            out.put("score", 4, sc);
        }
        if (in.has("save") && in["save"].scalar<int32_t>() != 0) {
            const std::string tmp = std::string(argv[2]) + ".voc";
            voc.saveToBinaryFile(tmp);
            std::vector<uint8_t> bytes;
            if (FILE *f = fopen(tmp.c_str(), "rb")) {
                uint8_t buf[4096];
                size_t got;
                while ((got = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
                fclose(f);
            }
            remove(tmp.c_str());
            out.put("saved", 0, bytes);
        }
        out.save(argv[2]);
    } catch (const std::exception &e) {
        fprintf(stderr, "dbow2_ref: %s\n", e.what());
        return 1;
    }
    return 0;
}
