// Extension: the projection model of a camera.  A Camera keeps its five numbers (fx, fy, cx, cy, bf); the model and its
// coefficients ride next to it, on the edge or the edge set, as the sensor pose does (BaseEdge::setCameraModel).
//   Pinhole         pu = fx X / Z + cx,  pv = fy Y / Z + cy                                   (the default)
//   KannalaBrandt   theta = atan2(sqrt(X^2 + Y^2), Z),  theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
//                   pu = fx theta_d X / r + cx,  pv = fy theta_d Y / r + cy                   (fisheye, "equidistant";
//                   ORB-SLAM3's KannalaBrandt8, OpenCV's cv::fisheye).  Points with Z <= 0 are legal.
// No HIP/CUDA header is pulled in here.
#pragma once
#include "cugo_types.h"

namespace cugo
{

enum CameraModelType : int
{
    Pinhole = 0,
    KannalaBrandt = 1
};

struct CameraModel
{
    CameraModelType type = Pinhole;
    Scalar k[4] = {}; // k1..k4; not looked at for Pinhole
    CameraModel() = default;
    CameraModel(CameraModelType type_, Scalar k1, Scalar k2, Scalar k3, Scalar k4) : type(type_), k{k1, k2, k3, k4} {}
};

} // namespace cugo
