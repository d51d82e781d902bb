// StateValidChecker and its base collisionDetection at the reference's signatures (include/StateValidChecker.h:47-150,
// include/collisions.h:43-68), for the planner's call sites that stay as they are -- RRT* (src/myRRTstar.cc:302-464) calls
// checkMotionTW and MotionCost for one pair of states at a time, Planning.cc:190 calls isValid -- and with batch members for the
// call sites that can hand over all the neighbours of a new node at once: checkMotionsTW and MotionCosts.  INTEGRATION.md has the
// mapping.
//
// An object owns one C-ABI handle (aos2_svc_t, shared by its copies): the obstacles and the camera's map go up once, and every
// later call is one C-ABI call.  The arithmetic is csrc/motion_tw.h's on both sides of the ABI: sin, cos and atan2 are its fixed
// operation sequences, not libm's, so a path built here one motion at a time and one built in a batch agree bit for bit.
// A state whose component is not finite, or whose heading is beyond +-1e4, ends the process like every failed call of these
// classes (aos2_handles.h).
//
// The ob::State* overloads are templates over anything with `values[i]` (ob::RealVectorStateSpace::StateType is one), so that
// this header needs no OMPL.  Left out, on purpose:
//   checkMotionStraightLine (src/StateValidChecker.cc:52-72) hands a Vector of size 2 to check_collisions, which reads q[2]
//     (src/collisions.cc:77): undefined behaviour in the reference, with no result to reproduce.
//   checkMotion / reconstructMotion (:121-182) ask the OMPL state space for validSegmentCount and interpolate; their states can be
//     checked in one call with isValidBatch.
//   collisionDetection() with load_obstacles (src/collisions.cc:10-21, :39-64): a caller reads the file and uses
//     collisionDetection(ppMatrix); print_obs, kNeighbors and the kd-tree: no caller outside the class.
//   defaultSettings, retrieveStateVector, updateStateVector, the print and log members: OMPL plumbing and console output.
// Include AFTER the headers that declare cv::Mat and map_data (the reference's, or tests/cpp/refstub/state_valid_checker_stub.h).
#pragma once
#include <memory>
#include <vector>

#include "../csrc/motion_tw.h"
#include "camera.h"

typedef std::vector<std::vector<double> > ppMatrix;
typedef std::vector<double> Vector;
typedef std::vector<int> VectorInt;

typedef struct {
    bool valid;
    VectorInt v;
    Vector w;
    Vector t;
} TW_path_data;

class collisionDetection {
public:
    collisionDetection(ppMatrix FloorMap)
    {
        aos2_svc_t *h = nullptr;
        aos2::check(aos2_svc_create(aos2::thread_device(), &h), "collisionDetection");
        mSvc.reset(h, aos2_svc_destroy);
        aos2::check(aos2_svc_params_default(&mParams), "collisionDetection");
        std::vector<double> xy;
        xy.reserve(2 * FloorMap.size());
        for (size_t i = 0; i < FloorMap.size(); ++i) {
            xy.push_back(FloorMap[i][0]);
            xy.push_back(FloorMap[i][1]);
        }
        aos2::check(aos2_svc_set_obstacles(h, (int)FloorMap.size(), xy.data(), obs_r), "collisionDetection");
    }

    // true if the robot is not in collision with the obstacles (and inside the bounds, as src/collisions.cc:77 tests them)
    bool check_collisions(Vector q, double robot_radius)
    {
        aos2_svc_params_t p = mParams;
        p.robot_r = robot_radius;
        aos2::check(aos2_svc_set_params(mSvc.get(), &p), "collisionDetection::check_collisions");
        uint8_t valid = 0, free_ = 0;
        aos2::check(aos2_svc_valid(mSvc.get(), 1, q.data(), &valid, &free_, nullptr), "collisionDetection::check_collisions");
        return free_ != 0;
    }

protected:
    std::shared_ptr<aos2_svc_t> mSvc;
    aos2_svc_params_t mParams;    // what the derived class sends before a call

private:
    double obs_r = 0.1;           // assumed point obstacle radius, include/collisions.h:61
};

class StateValidChecker : public collisionDetection, public camera {
public:
    StateValidChecker(map_data MD, ppMatrix FloorMap, int thres = 20) : collisionDetection(FloorMap), camera(MD, thres), StartState(3)
    {
        LoadInto(aos2_svc_vis(mSvc.get()));
    }
    StateValidChecker(ppMatrix FloorMap) : collisionDetection(FloorMap), StartState(3) { LoadInto(aos2_svc_vis(mSvc.get())); }

    // ---- a state
    bool isValid(Vector q)
    {
        uint8_t valid = 0;
        aos2::check(aos2_svc_valid(Handle(), 1, q.data(), &valid, nullptr, nullptr), "StateValidChecker::isValid");
        return valid != 0;
    }
    template <class State>
    bool isValid(const State *state)
    {
        return isValid(Retrieve(state));
    }
    // isValid of every row of Q in one call (no reference equivalent)
    std::vector<bool> isValidBatch(const ppMatrix &Q)
    {
        const std::vector<double> s = Flatten(Q);
        std::vector<uint8_t> valid(Q.size());
        aos2::check(aos2_svc_valid(Handle(), (int)Q.size(), s.data(), valid.data(), nullptr, nullptr), "StateValidChecker::isValidBatch");
        return std::vector<bool>(valid.begin(), valid.end());
    }

    // ---- the two-wheel shortest path
    TW_path_data GetShortestPath(Vector q1, Vector q2) const
    {
        uint8_t ok = 0;
        int32_t type = -1;
        double t[3];
        aos2_svc_motions_out_t out = aos2_svc_motions_out_t();
        out.path_valid = &ok; out.type = &type; out.t = t;
        aos2::check(aos2_svc_motions(Handle(), 1, q1.data(), q2.data(), &out), "StateValidChecker::GetShortestPath");
        TW_path_data vwt;
        vwt.valid = ok != 0;
        if (!vwt.valid) return vwt;
        int s1, s2, dir;
        aos2::tw_candidate(type, s1, s2, dir);
        vwt.t = {t[0], t[1], t[2]};
        vwt.v = {dir, dir, dir};
        vwt.w = {s1 * vwt.v[0] / turn_radius, 0, s2 * vwt.v[2] / turn_radius};
        return vwt;
    }
    Vector myprop(Vector q, double vi, double wi, double ti) const
    {
        double out[3];
        aos2::tw_myprop(q.data(), vi, wi, ti, out);
        return {out[0], out[1], out[2]};
    }

    // ---- a motion
    bool checkMotionTW(Vector q1, Vector q2)
    {
        uint8_t valid = 0;
        aos2_svc_motions_out_t out = aos2_svc_motions_out_t();
        out.valid = &valid;
        aos2::check(aos2_svc_motions(Handle(), 1, q1.data(), q2.data(), &out), "StateValidChecker::checkMotionTW");
        return valid != 0;
    }
    bool reconstructMotionTW(Vector q1, Vector q2, ppMatrix &Q)
    {
        std::vector<ppMatrix> all;
        const std::vector<bool> ok = reconstructMotionsTW(ppMatrix(1, q1), ppMatrix(1, q2), all);
        if (!ok[0]) return false;   // (the reference returns before it pushes q1, :280-283)
        Q.insert(Q.end(), all[0].begin(), all[0].end());
        return true;
    }
    double MotionCost(Vector q1, Vector q2, const int cost_type = 1) const { return MotionCosts(ppMatrix(1, q1), ppMatrix(1, q2), cost_type)[0]; }
    template <class State>
    bool checkMotionTW(const State *s1, const State *s2)
    {
        return checkMotionTW(Retrieve(s1), Retrieve(s2));
    }
    template <class State>
    bool reconstructMotionTW(const State *s1, const State *s2, ppMatrix &Q)
    {
        return reconstructMotionTW(Retrieve(s1), Retrieve(s2), Q);
    }
    template <class State>
    double MotionCost(const State *s1, const State *s2, const int cost_type = 1) const
    {
        return MotionCost(Retrieve(s1), Retrieve(s2), cost_type);
    }

    double MotionCostLength(ppMatrix Q) const
    {
        double C = 0;
        for (size_t i = 1; i < Q.size(); i++) C += aos2::tw_length_term(Q[i - 1].data(), Q[i].data());
        return C;
    }
    double MotionCostCamera(ppMatrix Q) const
    {
        if (Q.empty()) return 0;   // (the reference's Q.size()-1 underflows there)
        std::vector<float> s;
        for (size_t i = 0; i < Q.size(); ++i)
            for (int k = 0; k < 3; ++k) s.push_back((float)Q[i][k]);
        const int32_t off[2] = {0, (int32_t)Q.size()};
        double cost = 0;
        aos2::check(aos2_vis_motion_costs(aos2_svc_vis(Handle()), 1, off, s.data(), feature_threshold, &cost), "StateValidChecker::MotionCostCamera");
        return cost;
    }

    // ---- batch members (no reference equivalent): row k of q1 with row k of q2, all in one call
    std::vector<bool> checkMotionsTW(const ppMatrix &q1, const ppMatrix &q2)
    {
        std::vector<uint8_t> valid(q1.size());
        aos2_svc_motions_out_t out = aos2_svc_motions_out_t();
        out.valid = valid.data();
        Motions(q1, q2, out, "StateValidChecker::checkMotionsTW");
        return std::vector<bool>(valid.begin(), valid.end());
    }
    // cost_type: 1 - motion length, 2 - number of visible features (:543-578); anything else gives zeros (the reference falls off
    // the end of its switch there)
    std::vector<double> MotionCosts(const ppMatrix &q1, const ppMatrix &q2, const int cost_type = 1) const
    {
        std::vector<double> cost(q1.size(), 0.0);
        aos2_svc_motions_out_t out = aos2_svc_motions_out_t();
        if (cost_type == 1) out.cost_length = cost.data();
        if (cost_type == 2) out.cost_camera = cost.data();
        Motions(q1, q2, out, "StateValidChecker::MotionCosts");
        return cost;
    }
    // reconstructMotionTW of every pair: Q[k] is empty where it returns false
    std::vector<bool> reconstructMotionsTW(const ppMatrix &q1, const ppMatrix &q2, std::vector<ppMatrix> &Q) const
    {
        const size_t nm = q1.size();
        std::vector<uint8_t> ok(nm);
        std::vector<int32_t> n_states(nm), off(nm + 1);
        aos2_svc_motions_out_t out = aos2_svc_motions_out_t();
        out.n_states = n_states.data();
        Motions(q1, q2, out, "StateValidChecker::reconstructMotionsTW");   // the sizes first
        std::vector<double> states(3 * (size_t)out.states_needed + 3);
        out.path_valid = ok.data(); out.offsets = off.data(); out.states = states.data(); out.states_capacity = out.states_needed;
        Motions(q1, q2, out, "StateValidChecker::reconstructMotionsTW");
        Q.assign(nm, ppMatrix());
        for (size_t k = 0; k < nm; ++k)
            for (int32_t i = off[k]; ok[k] && i < off[k + 1]; ++i) Q[k].push_back({states[3 * (size_t)i], states[3 * (size_t)i + 1], states[3 * (size_t)i + 2]});
        return std::vector<bool>(ok.begin(), ok.end());
    }

    /** Misc */
    double normDistance(Vector a1, Vector a2, int d = -1) const
    {
        if (d == -1) d = (int)a1.size();
        return aos2::tw_norm_distance(a1.data(), a2.data(), d);
    }
    const int n = 3;   // State dimension
    int get_n() { return n; }
    double get_maxDistHeuristicValidity() { return maxDistHeuristicValidity; }
    template <class State>
    void setStartState(State *st)
    {
        StartState = Retrieve(st);
    }
    Vector getStartState() { return StartState; }
    Vector StartState;
    // heuristicValidityCheck is private and false in every constructor of the reference; this is the only way to turn it on
    void setHeuristicValidityCheck(bool on) { heuristicValidityCheck = on; }

private:
    template <class State>
    Vector Retrieve(const State *state) const
    {
        Vector q(n);
        for (int i = 0; i < n; i++) q[i] = state->values[i];
        return q;
    }
    static std::vector<double> Flatten(const ppMatrix &Q)
    {
        std::vector<double> s;
        s.reserve(3 * Q.size());
        for (size_t i = 0; i < Q.size(); ++i) s.insert(s.end(), Q[i].begin(), Q[i].begin() + 3);
        return s;
    }
    // the handle with this object's parameters as they stand (the members are plain fields: they may have been changed)
    aos2_svc_t *Handle() const
    {
        aos2_svc_params_t p = mParams;
        p.turn_radius = turn_radius; p.robot_r = robot_r; p.dt = dt;
        p.heuristic = heuristicValidityCheck ? 1 : 0;
        p.max_dist_heuristic = maxDistHeuristicValidity;
        for (int i = 0; i < 3; ++i) p.start[i] = StartState[i];
        p.feature_threshold = feature_threshold;
        aos2::check(aos2_svc_set_params(mSvc.get(), &p), "StateValidChecker");
        return mSvc.get();
    }
    void Motions(const ppMatrix &q1, const ppMatrix &q2, aos2_svc_motions_out_t &out, const char *what) const
    {
        if (q1.size() != q2.size()) {
            std::cerr << what << ": q1 and q2 differ in length" << std::endl;
            std::exit(-1);
        }
        const std::vector<double> a = Flatten(q1), b = Flatten(q2);
        aos2::check(aos2_svc_motions(Handle(), (int)q1.size(), a.data(), b.data(), &out), what);
    }

    bool heuristicValidityCheck = false;
    double maxDistHeuristicValidity = 2;   // MAX_DIST_HEURISTIC
    double robot_r = 0.4;                  // ROBOT_RADIUS
    double turn_radius = 0.25;             // TURN_RADIUS
    double dt = 0.3;                       // DT
};
