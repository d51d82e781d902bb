// TEST INFRASTRUCTURE: as much of Eigen::Quaterniond, Eigen::Vector3d and g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) as
// active-orb-slam2_amd/host/OptimizeSim3.h touches, with the real names and argument orders, so that it compiles in an image without
// Eigen: Quaterniond(w, x, y, z) with x() .. w(), Vector3d(x, y, z) with operator[], Sim3(r, t, s) with rotation(), translation(),
// scale().  No arithmetic.  In a real build these come from <Eigen/Geometry> and "Thirdparty/g2o/g2o/types/sim3.h".
#pragma once

namespace Eigen {

class Quaterniond {
public:
    Quaterniond() = default;
    Quaterniond(double w, double x, double y, double z) : c_{x, y, z, w} {}
    double x() const { return c_[0]; }
    double y() const { return c_[1]; }
    double z() const { return c_[2]; }
    double w() const { return c_[3]; }

private:
    double c_[4] = {0, 0, 0, 1};
};

class Vector3d {
public:
    Vector3d() = default;
    Vector3d(double x, double y, double z) : v_{x, y, z} {}
    double operator[](int i) const { return v_[i]; }
    double &operator[](int i) { return v_[i]; }

private:
    double v_[3] = {0, 0, 0};
};

}  // namespace Eigen

namespace g2o {

struct Sim3 {
    Sim3() = default;
    Sim3(const Eigen::Quaterniond &r_, const Eigen::Vector3d &t_, double s_) : r(r_), t(t_), s(s_) {}
    const Eigen::Vector3d &translation() const { return t; }
    const Eigen::Quaterniond &rotation() const { return r; }
    const double &scale() const { return s; }

protected:
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s = 1.;
};

}  // namespace g2o
