// Extension: the radial-tangential lens distortion of a pinhole camera (OpenCV's distCoeffs = (k1, k2, p1, p2, k3),
// Kalibr's and EuRoC's radtan, ROS's plumb_bob, ORB-SLAM's Camera.k1 .. p2, k3).  A Camera keeps its five numbers (fx,
// fy, cx, cy, bf); the coefficients ride next to it, on the edge or the edge set, as the sensor pose and the projection
// model do (BaseEdge::setDistortion).  With a = X / Z, b = Y / Z, r2 = a^2 + b^2:
//   a' = a (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 a b + p2 (r2 + 2 a^2)
//   b' = b (1 + k1 r2 + k2 r2^2 + k3 r2^3) + p1 (r2 + 2 b^2) + 2 p2 a b
//   pu = fx a' + cx,  pv = fy b' + cy
// Measurements on a distorted camera are RAW pixels: nothing is undistorted on the way in.  All zeros (the default) is
// the plain pinhole.  No HIP/CUDA header is pulled in here.
#pragma once
#include "cugo_types.h"

namespace cugo
{

struct CameraDistortion
{
    Scalar k1 = 0, k2 = 0, p1 = 0, p2 = 0, k3 = 0;
    CameraDistortion() = default;
    CameraDistortion(Scalar k1_, Scalar k2_, Scalar p1_, Scalar p2_, Scalar k3_) : k1(k1_), k2(k2_), p1(p1_), p2(p2_), k3(k3_) {}
    /** no distortion: every coefficient is exactly zero (a NaN is not zero: initialize() gets to refuse it) */
    bool isZero() const noexcept { return k1 == 0 && k2 == 0 && p1 == 0 && p2 == 0 && k3 == 0; }
};

} // namespace cugo
